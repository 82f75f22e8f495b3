"""Device filter against the only way to the same result without it
(DESIGN.md §8): on the table of one pass over a corpus in HBM, for four
predicates --

  min2    min_count = 2
  stop    a stop list of the table's 100 most frequent words
  prefix  a 2-byte prefix (the first two bytes of the table's most frequent
          word of at least two bytes)
  dry     min_count = 2 with MOX_FILTER_COUNT_ONLY (nothing is written)

-- the wall time of

  (a) Engine.filter_result(...)   -- the subset becomes the resident result
  (b) Engine.fetch() + the same predicate on the host + reduce_pairs of the
      kept words (mox_reduce_pairs on numpy arrays, no Python lists), which
      puts the subset back on the device; for `dry`, fetch + predicate only

on the same engine and table.  A filter replaces the result, so every timed
call is preceded by an untimed pass over the corpus that restores it; (a) and
(b) alternate, REPS times (REPS_BIG on a large table) after WARMUP warm-ups of each.  The host predicates
are numpy expressions over the fetched arrays (counts >= 2; the two prefix
bytes gathered at the offsets); the stop list is a Python set over the words,
so its (b) is measured on tables of at most HOST_LIST_MAX words and reported
as not measured above that.  (a)'s kept table is compared with (b)'s as
dictionaries in the same process.

  python tools/filter_timing.py [bytes] [zipf|hicard ...] [noalt]
  rocprofv3 --kernel-trace --stats -d DIR -- python tools/filter_timing.py BYTES hicard noalt   (per-kernel times)
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

REPS, WARMUP = 5, 1
REPS_BIG = 3  # repetitions on a table of more than HOST_LIST_MAX words ((b) takes seconds there)
HOST_LIST_MAX = 4 << 20
TABLES = {"zipf": (corpus.ZIPF, corpus.CONFIGS["C2"]["seed"]), "hicard": (corpus.HICARD, corpus.CONFIGS["C4"]["seed"])}


def stat(ts):
    return statistics.median(ts), min(ts), max(ts)


def host_mask(name, pred, counts, offs, data):
    """The predicate over the fetched arrays as a boolean mask."""
    if name in ("min2", "dry"):
        return counts >= 2
    if name == "prefix":
        p = pred["prefix"]
        lens = np.diff(offs.astype(np.int64))
        buf = np.frombuffer(data, dtype=np.uint8)
        o = offs[:-1].astype(np.int64)
        ok = lens >= 2
        safe = np.where(ok, o, 0)
        return ok & (buf[safe] == p[0]) & (buf[safe + 1] == p[1])
    stop = set(pred["drop"])
    ol = offs.tolist()
    return np.fromiter((data[x:y] not in stop for x, y in zip(ol, ol[1:])), dtype=bool, count=len(ol) - 1)


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

    def restore():
        e.run_device(d, nbytes)

    restore()
    t = e.fetch()
    counts, offs, data = t.arrays()
    n, nb = t.n, int(offs[-1])
    t.close()
    order = np.argsort(-counts.astype(np.int64), kind="stable")
    top = [data[int(offs[i]):int(offs[i + 1])] for i in order[:100]]
    two = next(w for w in top if len(w) >= 2)[:2]
    preds = {"min2": dict(min_count=2), "stop": dict(drop=top), "prefix": dict(prefix=two), "dry": dict(min_count=2, count_only=True)}
    del counts, offs, data, order
    res = {"table": name, "corpus_bytes": nbytes, "words": n, "word_bytes": nb, "table_bytes": 16 * n + 8 + nb,
           "prefix": two.decode("utf-8", "replace"), "cases": {}}

    def filt(pred):
        restore()
        t0 = time.perf_counter()
        info = e.filter_result(**pred)
        return (time.perf_counter() - t0) * 1e3, info

    def host_path(pname, pred):
        restore()
        t0 = time.perf_counter()
        t = e.fetch()
        counts, offs, data = t.arrays()
        t1 = time.perf_counter()
        mask = host_mask(pname, pred, counts, offs, data)
        kept = int(mask.sum())
        t2 = time.perf_counter()
        if pname != "dry":
            kb, ko, kc = pack_kept(mask, counts, offs, data)
            t3 = time.perf_counter()
            e._c(e._L.mox_reduce_pairs(e._h, ctypes.c_void_p(kb.ctypes.data if kb.size else None), ctypes.c_void_p(ko.ctypes.data),
                                       ctypes.c_void_p(kc.ctypes.data), kc.size))
            t4 = time.perf_counter()
        else:
            t3 = t4 = t2
        t.close()
        return {"total": (t4 - t0) * 1e3, "fetch": (t1 - t0) * 1e3, "predicate": (t2 - t1) * 1e3, "pack": (t3 - t2) * 1e3,
                "reduce_pairs": (t4 - t3) * 1e3, "kept": kept}

    def resident():
        t = e.fetch()
        try:
            return t.as_dict() if t.n <= HOST_LIST_MAX else (t.n, t.tokens, int(t.arrays()[1][-1]))
        finally:
            t.close()

    for pname, pred in preds.items():
        do_alt = alt and (pname != "stop" or n <= HOST_LIST_MAX)
        for _ in range(WARMUP):
            filt(pred)
            if do_alt:
                host_path(pname, pred)
        a, b, parts, info = [], [], [], None
        for _ in range(REPS if n <= HOST_LIST_MAX else REPS_BIG):  # interleaved: (a), (b), (a), (b), ...
            ms, info = filt(pred)
            a.append(ms)
            if do_alt:
                h = host_path(pname, pred)
                b.append(h["total"])
                parts.append(h)
        case = {"filter_ms": stat(a), "filter_ms_all": a, "info": {k: v for k, v in info.items() if k != "ms"}}
        line = "%-6s n=%d %-6s (a) filter %.3f ms (%.3f-%.3f) kept %d words / %d bytes" % (
            name, n, pname, *stat(a), info["words_kept"], info["bytes_kept"])
        if do_alt:
            med = {k: statistics.median(p[k] for p in parts) for k in ("fetch", "predicate", "pack", "reduce_pairs")}
            case.update({"host_ms": stat(b), "host_ms_all": b, "host_parts_median_ms": med})
            line += "  (b) fetch %.1f + predicate %.1f + pack %.1f + reduce_pairs %.1f = %.1f ms (%.1f-%.1f)  (b)/(a) %.1fx" % (
                med["fetch"], med["predicate"], med["pack"], med["reduce_pairs"], *stat(b), stat(b)[0] / stat(a)[0])
            assert parts[-1]["kept"] == info["words_kept"], "the host predicate keeps other words"
            if pname != "dry":  # the two kept tables: as dictionaries, or by their sizes and tokens where more than HOST_LIST_MAX words are kept
                want = resident()  # (b)'s, left by the last host_path
                filt(pred)
                assert resident() == want, "filter differs from the host path"
                line += "  tables equal" if info["words_kept"] <= HOST_LIST_MAX else "  words, bytes and tokens equal"
        else:
            line += "  (b) not measured"
        res["cases"][pname] = case
        print(line, flush=True)
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
