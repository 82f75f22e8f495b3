// The body of k_reduce, compiled twice by mox_kernels.hip: as k_reduce
// (MOX_RED_ZERO 0: every ordinary pass) and as k_reduce_z (MOX_RED_ZERO 1: the
// reduce-only passes whose weighted records may hold a count of 0, which the
// table's publication protocol cannot take; see red_zero).  Two separate kernels
// rather than a runtime switch: k_reduce is register-tight (64 VGPRs, measured
// spills) and stays exactly the code it was.
extern "C" __global__ __launch_bounds__(RED_THREADS, 8) void MOX_RED_KERNEL(Work w) {  // 8 waves per SIMD: 2 workgroups per CU
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  RedLds s;
  uint8_t* sp = smem;
  s.tag4 = (uint4*)sp; sp += RED_SLOTS * 4;
  s.key = (uint4*)sp; sp += RED_SLOTS * 16;
  s.cnt = (unsigned long long*)sp; sp += RED_SLOTS * 8;
  s.idx = (uint16_t*)sp; sp += RED_CAP * 2;
  s.bin = (uint16_t*)sp; sp += (RED_SORTB + 8) * 2;
  s.fill = (uint16_t*)sp; sp += RED_SORTB * 2;
  s.misc = (uint32_t*)sp; sp += 16;
  __shared__ uint32_t dbgc[8];
  __shared__ uint32_t s_unit;
  __shared__ uint64_t red_wsum[RED_THREADS / 64];
  uint32_t* rpre = reinterpret_cast<uint32_t*>(s.idx);  // region prefix (G + 1 words in the idx + bin space)
  uint16_t* rtab = s.fill;                              // ticket -> region (fill space: free until the sort)
  static_assert(RED_CAP * 2 + (RED_SORTB + 8) * 2 >= (MAX_MAP_GRID + 1) * 4, "region prefix space");
  s.dbg = MOX_ABL(w.dbg, DBG_COUNT) ? dbgc : nullptr;
  s.plain = MOX_ABL(w.dbg, DBG_RED_PLAINADD) != 0;
  s.ctl = w.ctl;
  if (threadIdx.x < 8) dbgc[threadIdx.x] = 0;
  const int tid = threadIdx.x, lane = tid & 63;
  const uint32_t G = reg_grid(w), RC = reg_cap(w);  // cold regions per partition (<= MAX_MAP_GRID), records per region
  uint32_t* tags = reinterpret_cast<uint32_t*>(s.tag4);
  // an overflowed map, directory or split means this attempt is rerun with
  // larger buffers: its records are incomplete (nothing downstream reads them)
  if (w.ctl->overflow & OVF_RERUN) return;
  // workgroup b < NB first reduces partition b if it was not split (no queue),
  // then all workgroups take oversized sub-buckets from the work list
  const uint32_t NBIG = (uint32_t)w.ctl->n_big;
  uint32_t max_kk = 0;
#ifdef MOX_RED_STATS  // per-wave cycles: [0] between chunks (loop, load waits) [1] hash [2] fast path [3] slow path
  uint64_t rcyc[4] = {0, 0, 0, 0}, rprev = __builtin_amdgcn_s_memtime();
#define RED_MARK(k) do { const uint64_t t_ = __builtin_amdgcn_s_memtime(); rcyc[k] += t_ - rprev; rprev = t_; } while (0)
#else
#define RED_MARK(k) do { } while (0)
#endif
  const uint32_t ob = blockIdx.x < NB ? w.red_order[blockIdx.x] : 0u;  // k_unit_scan: biggest partitions first
  bool own = blockIdx.x < NB && w.b_kk[ob] == 0;
  for (;;) {
    uint32_t u;
    if (own) {
      u = w.u_base[ob];
      own = false;
    } else {
      if (tid == 0) {
        const uint32_t t = (uint32_t)atomicAdd(&w.ctl->red_ticket, 1ull);
        s_unit = t < NBIG ? w.big_units[t] : 0xFFFFFFFFu;
      }
      __syncthreads();
      u = s_unit;
      __syncthreads();
    }
    if (u == 0xFFFFFFFFu) break;
    const UnitDesc ud = w.udesc[u];
    const uint32_t b = ud.part;
    const bool split = ud.in_n != UNIT_WHOLE;
    const uint32_t shift0 = NB_LOG2 + ud.kk;
    uint64_t ws0, ws1;
    const WRec* wsrc;
    if (split) { wsrc = w.split_w; ws0 = ud.win_off; ws1 = ws0 + ud.win_n; }
    else { wsrc = w.w_sorted; ws0 = w.w_off[b]; ws1 = w.w_off[b + 1]; }
    const uint64_t out0 = ud.rec_off;
    // split unit: one contiguous cold range
    const uint64_t kin0 = split ? ud.in_off : 0;
    const uint32_t kin_n = split ? ud.in_n : 0;
    const bool stamp = MOX_ABL(w.dbg, DBG_STAMP) && tid == 0 && !split;
    if (stamp) w.stamps[b * 8 + 0] = __builtin_amdgcn_s_memrealtime();
    uint32_t kk = 0;
    uint64_t written = 0, wbytes = 0;
    bool failed = false;
    for (uint32_t sub = 0; sub < (1u << kk);) {
      for (int i = tid; i < RED_SLOTS; i += RED_THREADS) {
        tags[i] = 0;
        s.cnt[i] = 0;
      }
      if (tid == 0) { s.misc[0] = 0; s.misc[1] = 0; s.misc[2] = 0; s.misc[3] = 0; }
      // region prefix of a whole partition (the map workgroups' regions one after
      // another), in the sort index / bin space, which is free until the sort
      bool tab = false;  // ticket -> region table built
      if (!split) {
        uint64_t tot;
        const uint32_t cn = tid < (int)G ? cold_n_at(w, G, tid, b) : 0u;
        const uint64_t ex = block_exscan(cn, red_wsum, tot);
        if (tid < (int)G) rpre[tid] = (uint32_t)ex;
        if (tid == 0) rpre[G] = (uint32_t)tot;
        // region of every ticket start (record j RED_TICKET): the region holding
        // it, written by that region's thread from its own prefix and count, so
        // a wave finds a ticket's region in one LDS read instead of a binary
        // search over the prefix (8 dependent reads at 256 regions)
        tab = (tot + RED_TICKET - 1) / RED_TICKET <= (uint64_t)RED_TAB_MAX;
        if (tab && cn) {
          for (uint32_t j = (uint32_t)((ex + RED_TICKET - 1) / RED_TICKET); (uint64_t)j * RED_TICKET < ex + cn; j++)
            rtab[j] = (uint16_t)tid;
        }
      }
      __syncthreads();
      for (int rep = 0; rep < (MOX_ABL(w.dbg, DBG_RED_TWICE) ? 2 : 1); rep++)
      // cold records: the unit's records as one flat index space (whole
      // partition: region g = map workgroup g, at rpre[g]; split unit: one
      // contiguous range), handed to the waves in tickets of RED_TICKET records.
      // Each lane walks forward through the regions (its records ascend by 64
      // per step), the next chunks' loads in flight while the current one is
      // inserted.
      {
        if (rep) {  // DBG_RED_TWICE: the chunk tickets restart for the second stream
          __syncthreads();
          if (tid == 0) s.misc[2] = 0;
          __syncthreads();
        }
        const uint32_t n = split ? kin_n : rpre[G];
        constexpr uint32_t CH = 64 * RED_UNROLL;
        // in_sub as one masked compare: hash bits [32 - shift0 - kk, 32 - shift0)
        // equal sub (shift0 + kk <= 32 in every pass that runs; kk == 0: all)
        const uint32_t sub_mask = kk ? ((1u << kk) - 1u) << (32 - shift0 - kk) : 0u;
        const uint32_t sub_val = kk ? sub << (32 - shift0 - kk) : 0u;
        // dynamic shares: waves take the next chunks from an LDS ticket, so
        // they finish within a ticket of each other (static equal shares left
        // the slowest wave ~25 us behind per partition at C2,
        // profiles/r03_k_reduce_stamps.txt: insert_tail)
        constexpr uint32_t SCH = RED_TICKET;
        static_assert(RED_TICKET == 3 * CH, "a ticket is three chunks");
        const uint32_t a1 = n;
        auto grab = [&]() -> uint32_t {
          uint32_t v = 0;
          if (lane == 0) v = lds_fetch_add_lane(&s.misc[2], SCH);
          return __builtin_amdgcn_readfirstlane(v);
        };
        const uint32_t a0 = grab();
        const uint4* ubase = split ? w.split_k + kin0 : w.cold + b * RC;  // region g at + g NB RC
        const uint64_t gstride = (uint64_t)NB * RC;
        // lane state: region r holds flat records [rs, re).  (A per-lane 64-bit
        // region base instead of the multiply-add per load cost 2 VGPRs, which
        // at 64 VGPRs doubled the scratch spills.)
        uint32_t r = 0, rs = 0, re = split ? 0xFFFFFFFFu : 0u;
        auto seek = [&](uint32_t c) {  // region of record c: last r with rpre[r] <= c (wave-uniform search)
          if (split || c >= a1) return;
          if (tab) {  // c is a ticket start
            r = rtab[c / SCH];
          } else {
            uint32_t lo = 0, hi = G - 1;
            while (lo < hi) {
              const uint32_t mid = (lo + hi + 1) >> 1;
              if (rpre[mid] <= c) lo = mid; else hi = mid - 1;
            }
            r = lo;
          }
          rs = rpre[r];
          re = rpre[r + 1];
        };
        seek(a0);
        // the walk state is settled before the first record load: a value of it
        // still arriving from a register reload (scratch is vector memory) made
        // the compiler wait for every load in flight at each chunk (vmcnt(0))
        asm volatile("" ::"v"(r), "v"(rs), "v"(re));
        typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
        auto load = [&](uint32_t c, uint4 (&v)[RED_UNROLL]) {  // unconditional: uniform vmcnt
          // every address first, then the loads back to back: a region walk
          // between two loads of one chunk made the compiler wait for the first
          // (its temporaries reused the in-flight load's registers)
          const uint4* p[RED_UNROLL];
#pragma unroll
          for (int u2 = 0; u2 < RED_UNROLL; u2++) {
            const uint32_t i = c + u2 * 64 + lane;
            const bool ok = i < a1;
            bool adv = ok && i >= re;
            // per-lane walk to the region holding record i: one step covers a
            // chunk that crosses one region end (regions average ~150 records);
            // the loop only runs for regions of fewer than 64 records (the
            // compiler put a wait for every load in flight at the head of a
            // loop here, so the common step stays outside it)
            if (adv) { r++; rs = re; re = rpre[r + 1]; }
            adv = ok && i >= re;
            if (__any(adv)) {
              do {
                if (adv) { r++; rs = re; re = rpre[r + 1]; }
                adv = ok && i >= re;
              } while (__any(adv));
            }
            p[u2] = ok ? ubase + (uint64_t)r * gstride + (i - rs) : ubase;
          }
#pragma unroll
          for (int u2 = 0; u2 < RED_UNROLL; u2++) {
            const u32x4 x = *reinterpret_cast<const u32x4*>(p[u2]);
            v[u2] = make_uint4(x.x, x.y, x.z, x.w);
          }
        };
        auto process = [&](const uint4 (&cur)[RED_UNROLL], uint32_t c) {
          if (__hip_atomic_load(&s.misc[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) {  // redone anyway
            // the chunk's loads are waited for on this path too: left pending
            // into the next iteration, they made the compiler wait for every
            // load in flight (vmcnt(0)) before the region walk, each chunk
#pragma unroll
            for (int u2 = 0; u2 < RED_UNROLL; u2++) asm volatile("" ::"v"(cur[u2].x), "v"(cur[u2].y), "v"(cur[u2].z), "v"(cur[u2].w));
            return;
          }
          uint32_t h[RED_UNROLL];
          bool todo[RED_UNROLL];
          RED_MARK(0);
#pragma unroll
          for (int u2 = 0; u2 < RED_UNROLL; u2++) {
            h[u2] = hash32(cur[u2].x, cur[u2].y, cur[u2].z, cur[u2].w);
            todo[u2] = c + u2 * 64 + lane < a1 && ((h[u2] ^ sub_val) & sub_mask) == 0u;  // in_sub
          }
          RED_MARK(1);
          if (!MOX_ABL(w.dbg, DBG_RED_NOINSERT)) {
            uint32_t nnew = 0;
#pragma unroll
            for (int u2 = 0; u2 < RED_UNROLL; u2++) {
              int r = RED_MISS;
              if (todo[u2]) r = red_try(s, h[u2], cur[u2], 1);
              todo[u2] = todo[u2] && r == RED_MISS;
              nnew += (uint32_t)__popcll(__ballot(r == RED_NEW));
            }
            // the chunk's new keys counted at once (one lane, one LDS atomic);
            // past RED_CAP the unit is redone in sub-passes.  No returning
            // atomic: -0.8 % against a per-chunk test of the returned count
            // (profiles/r05/k_reduce_lazycap_ab.txt)
            if (nnew && lane == 0) {
              lds_add_lane(&s.misc[0], nnew);  // the RED_CAP test once the stream is done
            }
            RED_MARK(2);
#pragma unroll
            for (int u2 = 0; u2 < RED_UNROLL; u2++)
              if (todo[u2] && !MOX_ABL(w.dbg, DBG_RED_NOSLOW)) {
                if (s.dbg) atomicAdd(&s.dbg[3], 1u);  // cold-stream lanes on the slow path
                red_insert(s, h[u2], cur[u2], 1);
              }
            RED_MARK(3);
          } else {
#pragma unroll
            for (int u2 = 0; u2 < RED_UNROLL; u2++) asm volatile("" ::"v"(h[u2]));
          }
        };
        uint32_t c = a0;
        uint4 A[RED_UNROLL], B[RED_UNROLL];
        // tickets of three chunks [c, c + CH), [c + CH, c + 2 CH), [c + 2 CH,
        // c + 3 CH): two chunks' loads in flight while one is inserted (the
        // stream is bound by the bytes each wave keeps in flight)
        uint4 C[RED_UNROLL];
        if (c < a1) {
          load(c, A);
          load(c + CH, B);
        }
        while (c < a1) {
          load(c + 2 * CH, C);
          uint32_t tv = 0;
          if (lane == 0) tv = lds_fetch_add_lane(&s.misc[2], SCH);
          process(A, c);
          const uint32_t cn = __builtin_amdgcn_readfirstlane(tv);
          seek(cn);
          load(cn, A);
          process(B, c + CH);
          load(cn + CH, B);
          process(C, c + 2 * CH);
          c = cn;
        }
      }
      if (stamp) w.stamps[b * 8 + 1] = __builtin_amdgcn_s_memrealtime();  // wave 0 done streaming
      // A weighted record with count 0 (mox_reduce_pairs lets one through, and a
      // merge of two tables can hold the same such word twice) cannot go through
      // the table's protocol, where a count of 0 means "claimed, key not yet
      // published": a second record of its key would wait for a publication that
      // never comes.  k_reduce_z sets them aside here and places them after the
      // barrier below; k_reduce (every pass whose weighted counts are all > 0:
      // dictionary totals, spills, Unicode-lane words) compiles none of this.
#if MOX_RED_ZERO
      bool zero_seen = false;
#endif
      for (uint64_t i = ws0 + tid; i < ws1; i += RED_THREADS) {
        const WRec rr = wsrc[i];
#if MOX_RED_ZERO
        if (rr.count == 0) { zero_seen = true; continue; }
#endif
        const uint4 k = make_uint4((uint32_t)rr.w0, (uint32_t)(rr.w0 >> 32), (uint32_t)rr.w1, (uint32_t)(rr.w1 >> 32));
        const uint32_t h = hash32(k.x, k.y, k.z, k.w);
        if (!__hip_atomic_load(&s.misc[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) && in_sub(h, shift0, kk, sub)) {
          const int r = red_try(s, h, k, rr.count);
          if (r == RED_MISS) {
            red_insert(s, h, k, rr.count);
          } else if (r == RED_NEW) {
            const uint32_t u0 = atomicAdd(&s.misc[0], 1u);
            if (u0 >= (uint32_t)RED_CAP) s.misc[1] = 1;
          }
        }
      }
      // The chunks' new-key counts went out as inline-asm LDS adds, which the
      // compiler's wait-count tracking does not see: drain the DS queue
      // explicitly, so the barrier's release cannot be dropped as "nothing
      // pending" and misc[0] is settled when it is read below.
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#if !MOX_RED_ZERO
      __syncthreads();
#else
      if (__syncthreads_or(zero_seen ? 1 : 0)) {
        // The zero-count records: every other key is published by now, so one
        // wave places them one at a time (red_zero), with no publication to wait for.
        if (tid < 64 && !s.misc[1]) red_zero_records(s, wsrc, ws0, ws1, shift0, kk, sub);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __syncthreads();
      }
#endif
#ifdef MOX_CHECK
      {  // table invariants red_try relies on: every bucket's taken slots are a
         // prefix, and no key sits in two slots of its two buckets
        bool ok = true;
        for (int bk = tid; bk < RED_BUCKETS; bk += RED_THREADS) {
          for (int i = 0; i < 4; i++) {
            const uint32_t t = tags[4 * bk + i];
            if (t == 0) {
              for (int j = i + 1; j < 4; j++) ok = ok && tags[4 * bk + j] == 0;
              continue;
            }
            const int lim = bk + 1 < RED_BUCKETS ? 8 : 4;
            for (int j = i + 1; j < lim; j++)
              if (tags[4 * bk + j] == t && key_eq16(s.key[4 * bk + j], s.key[4 * bk + i])) ok = false;
          }
        }
        (void)MOX_CHK(w, ok, CHK_RED_TABLE);
      }
#endif
      if (s.misc[0] > (uint32_t)RED_CAP) {  // (uniform: every thread reads the settled count)
        __syncthreads();
        if (tid == 0) s.misc[1] = 1;
        __syncthreads();
      }
      if (s.misc[1]) {  // too many distinct keys for one table: split further, redo the unit
        kk++;
        // the redo does not see this attempt's keys (readers take a slot's key
        // only after its published count, and counts restart at 0; cleared
        // anyway, so no stale key ever sits in a slot being claimed)
        for (int i = tid; i < RED_SLOTS; i += RED_THREADS) s.key[i] = make_uint4(0, 0, 0, 0);
        __syncthreads();
        if (shift0 + kk > 32) {  // > RED_CAP distinct keys share every hash bit: cannot split
          if (tid == 0) atomicOr(&w.ctl->overflow, OVF_REDUCE);
          failed = true;
          break;
        }
        sub = 0;
        written = 0;
        wbytes = 0;
        continue;
      }
      // deterministic order (key_less): bucket sort by the hash bits below the
      // unit and sub-pass bits, then a key_less insertion sort inside each bin
      if (stamp) w.stamps[b * 8 + 2] = __builtin_amdgcn_s_memrealtime();  // all waves done inserting
      const uint32_t bsh = shift0 + kk;
      for (int i = tid; i < RED_SORTB; i += RED_THREADS) { s.bin[i] = 0; s.fill[i] = 0; }
      __syncthreads();
      for (int i = tid; i < RED_SLOTS; i += RED_THREADS)
        if (tags[i]) {
          const uint32_t bn = red_bin(tags[i], bsh);
          atomicAdd(reinterpret_cast<uint32_t*>(s.bin) + (bn >> 1), 1u << (16 * (bn & 1)));
        }
      __syncthreads();
      {  // exclusive scan of the RED_SORTB bin counts (2 per thread)
        uint64_t tot;
        const uint32_t c0 = s.bin[2 * tid], c1 = s.bin[2 * tid + 1];
        const uint64_t ex = block_exscan(c0 + c1, red_wsum, tot);
        s.bin[2 * tid] = (uint16_t)ex;
        s.bin[2 * tid + 1] = (uint16_t)(ex + c0);
        if (tid == 0) s.bin[RED_SORTB] = (uint16_t)tot;
      }
      __syncthreads();
      // distinct keys = taken slots (the tag count of the bin scan above), not
      // misc[0]: no wave may disagree on it (check builds: the two agree)
      const uint32_t nu = s.bin[RED_SORTB];
      (void)MOX_CHK(w, nu == s.misc[0], CHK_RED_NU);
      for (int i = tid; i < RED_SLOTS; i += RED_THREADS)
        if (tags[i]) {
          const uint32_t bn = red_bin(tags[i], bsh);
          const uint32_t old = atomicAdd(reinterpret_cast<uint32_t*>(s.fill) + (bn >> 1), 1u << (16 * (bn & 1)));
          const uint32_t p = s.bin[bn] + ((old >> (16 * (bn & 1))) & 0xFFFFu);
          s.idx[p] = (uint16_t)i;
        }
      __syncthreads();
      if (!MOX_ABL(w.dbg, DBG_RED_NOSORT)) {
        for (int bn = tid; bn < RED_SORTB; bn += RED_THREADS) {
          const uint32_t lo = s.bin[bn], hi = s.bin[bn + 1];
          for (uint32_t i = lo + 1; i < hi; i++) {  // insertion sort of a tiny bin
            const uint16_t x = s.idx[i];
            uint32_t j = i;
            while (j > lo && red_less(s, x, s.idx[j - 1])) { s.idx[j] = s.idx[j - 1]; j--; }
            s.idx[j] = x;
          }
        }
      }
      __syncthreads();
      if (stamp) w.stamps[b * 8 + 3] = __builtin_amdgcn_s_memrealtime();  // sorted
      uint32_t lb = 0;
      for (uint32_t i = tid; i < nu; i += RED_THREADS) {
        const uint16_t sl = s.idx[i];
        const uint4 kk4 = s.key[sl];
        // check builds: the unit's distinct keys stay inside its record range
        if (MOX_CHK(w, written + i < (split ? (uint64_t)ud.in_n + ud.win_n : w.rec_off[b + 1] - w.rec_off[b]) &&
                           out0 + written + i < w.uniq_cap, CHK_RED_OUT)) {
          w.uk[out0 + written + i] = kk4;
          w.uc[out0 + written + i] = s.cnt[sl];
        }
        lb += key_len16(kk4);
      }
      if (lb) atomicAdd(&s.misc[3], lb);
      written += nu;
      sub++;
      lds_barrier();  // the table is re-zeroed next: LDS only, the uk / uc stores need not land first
      if (tid == 0) wbytes += s.misc[3];  // read (and reset at the next sub-pass) by tid 0 only
    }
    if (stamp) {
      w.stamps[b * 8 + 4] = __builtin_amdgcn_s_memrealtime();
      uint32_t hw;
      asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
      w.stamps[b * 8 + 5] = hw;
      w.stamps[b * 8 + 6] = s.misc[0];
    }
    if (tid == 0) {
      w.u_uniq[u] = failed ? 0 : written;
      w.u_bytes[u] = failed ? 0 : wbytes;
      if (!split) w.b_uniq[b] = failed ? 0 : written;  // split partitions: summed by k_unit_uniq_scan
    }
    if (kk > max_kk) max_kk = kk;
    __syncthreads();
  }
#ifdef MOX_RED_STATS
  if (lane == 0 && w.stamps) {
    const int wv = tid >> 6;
    constexpr int NWV = RED_THREADS / 64;
    unsigned long long* o = w.stamps + 8 * 4096 + 8 * 1024 * MAP_WAVES + ((uint64_t)blockIdx.x * NWV + wv) * 4;
    for (int k = 0; k < 4; k++) o[k] = rcyc[k];
  }
#endif
  if (tid == 0) {
    if (max_kk) atomicMax(&w.ctl->max_sub, 1u << max_kk);
    if (s.dbg) for (int i = 0; i < 8; i++) atomicAdd(&w.ctl->dbg_cnt[i], (unsigned long long)dbgc[i]);
  }
}
