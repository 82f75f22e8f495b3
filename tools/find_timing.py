"""Device search of the sorted result against the streamed lookup and the
filter: on the table of one pass over a corpus in HBM, sorted on
the device (sort_result), the median and range of REPS calls after WARMUP
warm-ups of

  (a) Engine.find_packed(keys, "exact") and Engine.lookup_packed(keys) on the
      same keys in this process, interleaved, for q = 10, 10,000 and 1,048,576
      keys, half of them present (the counts are compared);
  (b) find(mode="prefix") for ten 3-byte prefixes;
  (c) find(mode="prefix") for one 1-byte prefix, with and without sums (its
      range holds whole tiles: the pass over the counts runs);
  (d) complete(prefix, 10) against filter_result(prefix) + top_words(10) on a
      second engine that holds the same pass's table (the filter replaces the
      result, so that engine runs the pass again before each repetition,
      outside the timed window; the ten counts are compared).

The keys are drawn with the corpus's own seed.

  python tools/find_timing.py [bytes] [zipf|hicard ...] [nofilter]
  rocprofv3 --kernel-trace --stats -d DIR -- python tools/find_timing.py BYTES hicard nofilter   (per-kernel times)
"""
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "map-oxidize_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mox  # noqa: E402
from mox import corpus  # noqa: E402
from lookup_timing import QS, REPS, TABLES, WARMUP, make_queries, median_ms  # noqa: E402


def interleaved_ms(fa, fb, reps=REPS, warmup=WARMUP):
    """(median, min, max) of fa and of fb, one call of each in turn."""
    for _ in range(warmup):
        fa()
        fb()
    ta, tb = [], []
    for _ in range(reps):
        for f, ts in ((fa, ta), (fb, tb)):
            t0 = time.perf_counter()
            f()
            ts.append((time.perf_counter() - t0) * 1e3)
    return tuple((statistics.median(ts), min(ts), max(ts)) for ts in (ta, tb))


def pack(words):
    o = np.zeros(len(words) + 1, dtype=np.uint64)
    np.cumsum([len(w) for w in words], out=o[1:])
    return np.frombuffer(b"".join(words), dtype=np.uint8), o


def load(kind, seed, nbytes):
    e = mox.Engine(device=0, reserve_bytes=nbytes)
    host = corpus.fill(kind, seed, 0, nbytes)
    d = e.alloc(nbytes)
    e.h2d(d, host)
    del host
    e.run_device(d, nbytes)
    return e, d


def measure(name, nbytes, with_filter):
    kind, seed = TABLES[name]
    e, d = load(kind, seed, nbytes)
    t0 = time.perf_counter()
    e.sort_result()
    sort_ms = (time.perf_counter() - t0) * 1e3
    t = e.fetch()
    counts, offs, data = t.arrays()
    n, nb = t.n, int(offs[-1])
    t.close()
    res = {"table": name, "corpus_bytes": nbytes, "words": n, "word_bytes": nb, "sort_ms": sort_ms, "q": {}}
    fmt = "%.3f ms (%.3f-%.3f)"
    # (a) exact search against the streamed lookup, same keys, same process
    for q in QS:
        _, qdata, qoffs = make_queries(offs, data, q, seed)
        got = {}

        def find():
            got["f"] = e.find_packed(qdata, qoffs, "exact")

        def look():
            got["l"] = e.lookup_packed(qdata, qoffs)

        f_ms, l_ms = interleaved_ms(find, look)
        first, last, sums = got["f"]
        assert np.array_equal(sums, got["l"]), "find(exact) sums differ from the lookup's counts"
        info = e.find_packed(qdata, qoffs, "exact", with_info=True)[3]
        res["q"][q] = {"find_ms": f_ms, "lookup_ms": l_ms, "ratio_lookup_over_find": l_ms[0] / f_ms[0], "matched": info["matched"]}
        print(("%-6s n=%d q=%d  find(exact) " + fmt + "  lookup " + fmt + "  lookup / find %.2f  matched %d")
              % ((name, n, q) + f_ms + l_ms + (l_ms[0] / f_ms[0], info["matched"])), flush=True)
    # (b), (c) prefixes taken from the table's own words
    buf = np.frombuffer(data, dtype=np.uint8)
    rng = np.random.default_rng(seed)
    three = []
    for i in rng.permutation(n)[:2000].tolist():
        w = buf[int(offs[i]):int(offs[i + 1])].tobytes()
        if len(w) >= 3 and w[:3] not in three:
            three.append(w[:3])
        if len(three) == 10:
            break
    pdata, poffs = pack(three)
    b_ms = median_ms(lambda: e.find_packed(pdata, poffs, "prefix"))
    info = e.find_packed(pdata, poffs, "prefix", with_info=True)[3]
    res["prefix3"] = {"ms": b_ms, "prefixes": [p.hex() for p in three], "info": info}
    print(("%-6s ten 3-byte prefixes: find(prefix) " + fmt + "  rows %d  tile pass %d") % ((name,) + b_ms + (info["rows"], info["tile_pass"])),
          flush=True)
    one = buf[int(offs[n // 2]):int(offs[n // 2]) + 1].tobytes()
    odata, ooffs = pack([one])
    c_ms = median_ms(lambda: e.find_packed(odata, ooffs, "prefix"))
    c0_ms = median_ms(lambda: e.find_packed(odata, ooffs, "prefix", with_sums=False))
    first, last, sums, info = e.find_packed(odata, ooffs, "prefix", with_info=True)
    lo, hi = int(first[0]), int(last[0])
    assert int(sums[0]) == int(counts[lo:hi].sum(dtype=np.uint64)), "the prefix's sum differs from the fetched counts'"
    res["prefix1"] = {"prefix": one.hex(), "ms_with_sums": c_ms, "ms_without_sums": c0_ms, "info": info}
    print(("%-6s one 1-byte prefix %r: with sums " + fmt + "  without " + fmt + "  rows %d  tile pass %d")
          % ((name, one) + c_ms + c0_ms + (info["rows"], info["tile_pass"])), flush=True)
    # (d) completion against filter + top-k on a second engine
    pre = three[0][:2]
    d_ms = median_ms(lambda: e.complete(pre, 10).close())
    t = e.complete(pre, 10)
    want = sorted(c for _, c in t.items())
    t.close()
    res["complete"] = {"prefix": pre.hex(), "ms": d_ms}
    print(("%-6s complete(%r, 10) " + fmt) % ((name, pre) + d_ms), flush=True)
    if with_filter:
        e2, d2 = load(kind, seed, nbytes)
        ts = []
        for r in range(WARMUP + REPS):
            if r:
                e2.run_device(d2, nbytes)
            t0 = time.perf_counter()
            e2.filter_result(prefix=pre)
            t = e2.top_words(10)
            ts.append((time.perf_counter() - t0) * 1e3)
            assert sorted(c for _, c in t.items()) == want, "filter + top_words counts differ from complete's"
            t.close()
        ts = ts[WARMUP:]
        f_ms = (statistics.median(ts), min(ts), max(ts))
        res["complete"]["filter_top_ms"] = f_ms
        res["complete"]["ratio_filter_over_complete"] = f_ms[0] / d_ms[0]
        print(("%-6s filter_result(prefix) + top_words(10) " + fmt + "  filter / complete %.1f") % ((name,) + f_ms + (f_ms[0] / d_ms[0],)),
              flush=True)
        e2.free(d2)
        e2.close()
    e.free(d)
    e.close()
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    args = sys.argv[1:]
    nbytes = int(args.pop(0)) if args and args[0].isdigit() else 1 << 30
    with_filter = "nofilter" not in args
    names = [a for a in args if a != "nofilter"] or ["zipf", "hicard"]
    for name in names:
        measure(name, nbytes, with_filter)
