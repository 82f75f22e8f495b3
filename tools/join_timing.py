"""Device join against the only way to the same answer without it (DESIGN.md
§8): a corpus in HBM is cut into a window, its first 1/16, and the rest; the
rest is counted and accumulated (the total T), the window is counted (the
result R), and for three uses --

  anti   join_total("anti"): the window's new words become the result
  total  join_total("semi", "total"): the known words with the total's counts
  dry    join_total("anti", count_only=True): the info alone

-- the wall time of

  (a) Engine.join_total(...)
  (b) fetch() of T (possible only while T is the result: after the pass over
      the rest) + fetch() of R + a host dictionary join + for `anti` and
      `total` reduce_pairs of the kept rows (numpy arrays, no Python lists),
      which puts the subset back on the device

on the same engine.  A join replaces the result, so every timed call is
preceded by an untimed pass that restores R (or T, for its fetch); (a) and (b)
alternate, REPS times after WARMUP warm-ups of each.  The host join is a Python
dict over T's words, so (b)'s join and reduce_pairs are measured where T holds
at most HOST_JOIN_MAX words; above that only the two fetches are timed, which
is what the join has to beat.  (a)'s info is compared with (b)'s counts.

Where R holds at most LOOKUP_MAX words the tool ends with one lookup of R's
words in T, so that a kernel trace of the run shows k_lk_stream next to
k_jn_stream over the same table:

  python tools/join_timing.py [bytes] [zipf|hicard ...] [noalt]
  rocprofv3 --kernel-trace --stats -d DIR -- python tools/join_timing.py BYTES hicard noalt   (per-kernel times)
"""
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "map-oxidize_amd"))
import mox  # noqa: E402
from mox import corpus  # noqa: E402

REPS, WARMUP = 3, 1
HOST_JOIN_MAX = 4 << 20
TABLES = {"zipf": (corpus.ZIPF, corpus.CONFIGS["C2"]["seed"]), "hicard": (corpus.HICARD, corpus.CONFIGS["C4"]["seed"])}
USES = {"anti": dict(mode="anti"), "total": dict(mode="semi", counts="total"), "dry": dict(mode="anti", count_only=True)}


def stat(ts):
    return statistics.median(ts), min(ts), max(ts)


def words_of(offs, data):
    ol = offs.tolist()
    return [data[x:y] for x, y in zip(ol, ol[1:])]


def pack_kept(mask, counts, offs, data):
    """(bytes, offs, counts) of the kept words, packed with numpy."""
    lens = np.diff(offs.astype(np.int64))[mask]
    new_offs = np.zeros(lens.size + 1, dtype=np.uint64)
    np.cumsum(lens, out=new_offs[1:])
    src = offs[:-1].astype(np.int64)[mask]
    idx = np.repeat(src - new_offs[:-1].astype(np.int64), lens) + np.arange(int(new_offs[-1]), dtype=np.int64)
    return np.frombuffer(data, dtype=np.uint8)[idx], new_offs, np.ascontiguousarray(counts[mask])


def measure(name, nbytes, alt):
    kind, seed = TABLES[name]
    e = mox.Engine(device=0, reserve_bytes=nbytes)
    host = corpus.fill(kind, seed, 0, nbytes)
    d = e.alloc(nbytes)
    e.h2d(d, host)
    del host
    cut = nbytes // 16

    def window():
        e.run_range(d, nbytes, 0, cut, False)

    def rest():
        e.run_range(d, nbytes, cut, nbytes, True)

    rest()
    t = e.fetch()
    tn, tb = t.n, int(t.arrays()[1][-1])
    t.close()
    e.accumulate()
    window()
    t = e.fetch()
    _, r_offs, r_data = t.arrays()
    rn, rb = t.n, int(r_offs[-1])
    t.close()
    host_join = alt and tn <= HOST_JOIN_MAX
    res = {"table": name, "corpus_bytes": nbytes, "window_bytes": cut, "r_words": rn, "r_word_bytes": rb, "t_words": tn, "t_word_bytes": tb,
           "t_table_bytes": 16 * tn + 8 + tb, "cases": {}}

    def join(use):
        window()
        t0 = time.perf_counter()
        info = e.join_total(**use)
        return (time.perf_counter() - t0) * 1e3, info

    def host_path(uname):
        rest()
        t0 = time.perf_counter()
        tt = e.fetch()
        t_counts, t_offs, t_data = tt.arrays()
        t1 = time.perf_counter()
        window()
        t2 = time.perf_counter()
        tr = e.fetch()
        counts, offs, data = tr.arrays()
        t3 = time.perf_counter()
        out = {"fetch_t": (t1 - t0) * 1e3, "fetch_r": (t3 - t2) * 1e3, "join": 0.0, "reduce_pairs": 0.0, "kept": None}
        if host_join:
            total = dict(zip(words_of(t_offs, t_data), t_counts.tolist()))
            got = [total.get(w) for w in words_of(offs, data)]
            held = np.fromiter((g is not None for g in got), dtype=bool, count=len(got))
            mask = ~held if uname != "total" else held
            t4 = time.perf_counter()
            out["join"] = (t4 - t3) * 1e3
            out["kept"] = int(mask.sum())
            if uname != "dry":
                kb, ko, kc = pack_kept(mask, counts, offs, data)
                if uname == "total":
                    kc = np.array([g for g in got if g is not None], dtype=np.uint64)
                e._c(e._L.mox_reduce_pairs(e._h, ctypes.c_void_p(kb.ctypes.data if kb.size else None), ctypes.c_void_p(ko.ctypes.data),
                                           ctypes.c_void_p(kc.ctypes.data), kc.size))
                out["reduce_pairs"] = (time.perf_counter() - t4) * 1e3
        tt.close()
        tr.close()
        out["total"] = out["fetch_t"] + out["fetch_r"] + out["join"] + out["reduce_pairs"]
        return out

    for uname, use in USES.items():
        for _ in range(WARMUP):
            join(use)
            if alt:
                host_path(uname)
        a, parts, info = [], [], None
        for _ in range(REPS):  # interleaved: (a), (b), (a), (b), ...
            ms, info = join(use)
            a.append(ms)
            if alt:
                parts.append(host_path(uname))
        case = {"join_ms": stat(a), "join_ms_all": a, "info": {k: v for k, v in info.items() if k != "ms"}}
        line = "%-6s R=%d T=%d %-5s (a) join %.3f ms (%.3f-%.3f) matched %d kept %d" % (
            name, rn, tn, uname, *stat(a), info["words_matched"], info["words_kept"])
        if alt:
            med = {k: statistics.median(p[k] for p in parts) for k in ("fetch_t", "fetch_r", "join", "reduce_pairs", "total")}
            case["host_parts_median_ms"] = med
            line += "  (b) fetch T %.1f + fetch R %.1f" % (med["fetch_t"], med["fetch_r"])
            if host_join:
                assert parts[-1]["kept"] == info["words_kept"], "the host join keeps other words"
                line += " + dict join %.1f + reduce_pairs %.1f = %.1f ms  (b)/(a) %.1fx" % (
                    med["join"], med["reduce_pairs"], med["total"], med["total"] / stat(a)[0])
            else:
                line += " (host join not measured: T has more than %d words)" % HOST_JOIN_MAX
            line += "  fetch T alone / (a) %.1fx" % (med["fetch_t"] / stat(a)[0])
        res["cases"][uname] = case
        print(line, flush=True)
    if rn <= mox.LOOKUP_MAX:  # the lookup's stream over the same T, for a kernel trace
        rest()
        t0 = time.perf_counter()
        _, li = e.lookup_packed(r_data, r_offs, with_info=True)
        res["lookup_ms"] = (time.perf_counter() - t0) * 1e3
        res["lookup_found"] = li["found"]
        print("%-6s lookup of R's %d words in T: %.3f ms, %d found" % (name, rn, res["lookup_ms"], li["found"]), flush=True)
    e.free(d)
    e.close()
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    args = sys.argv[1:]
    nbytes = int(args.pop(0)) if args and args[0].isdigit() else 1 << 30
    alt = "noalt" not in args
    names = [a for a in args if a != "noalt"] or ["zipf", "hicard"]
    for name in names:
        measure(name, nbytes, alt)
