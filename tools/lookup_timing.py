"""Device lookup against the fetch it replaces: on the table of
one pass over a corpus in HBM, for q = 10, 10,000 and 1,048,576 query words,
half of them present, the median wall time of

  (a) Engine.lookup_packed(queries)   -- the words go up, q counts come back
  (b) Engine.fetch()                  -- the whole table to the host
  (c) fetch() + a host dict over every word + the q dict lookups
                                      -- the only way to the counts without (a)

(a) and (b) over REPS repetitions after WARMUP warm-ups.  (c)'s dict is built
once per table (it does not depend on q, and takes seconds to minutes in
Python): (c) = that fetch + that build + the q lookups.  (a)'s counts are
compared with (c)'s in the same process.  Also timed: (a) for q = 10 on the
result sorted on the device (the case a binary search per query would serve),
and top_words(10), whose k_tk_hist / k_tk_ties give the session's streaming
rate in a kernel trace.  The query words are drawn with the corpus's own seed.

  python tools/lookup_timing.py [bytes] [zipf|hicard ...] [nomap]
  rocprofv3 --kernel-trace --stats -d DIR -- python tools/lookup_timing.py BYTES hicard nomap   (per-kernel times)
"""
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

REPS, WARMUP = 10, 2
QS = (10, 10000, 1 << 20)
TABLES = {"zipf": (corpus.ZIPF, corpus.CONFIGS["C2"]["seed"]), "hicard": (corpus.HICARD, corpus.CONFIGS["C4"]["seed"])}


def median_ms(fn, reps=REPS, warmup=WARMUP):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), min(ts), max(ts)


def make_queries(offs, data, q, seed):
    """q words packed (uint8 array, offs): q // 2 table words drawn without
    replacement where the table has that many, and as many absent ones (a table
    word with a \\x01 byte behind it: the table's length mix, one byte longer),
    shuffled."""
    rng = np.random.default_rng(seed)
    n = offs.size - 1
    half = q // 2
    pick = rng.choice(n, size=half, replace=half > n)
    buf = np.frombuffer(data, dtype=np.uint8)
    words = [buf[int(offs[i]):int(offs[i + 1])].tobytes() for i in pick]
    words += [w + b"\x01" for w in words] if q > 1 else []
    words = words[:q] if len(words) >= q else words + [b"\x01"] * (q - len(words))
    order = rng.permutation(q)
    words = [words[i] for i in order]
    o = np.zeros(q + 1, dtype=np.uint64)
    np.cumsum([len(w) for w in words], out=o[1:])
    return words, np.frombuffer(b"".join(words), dtype=np.uint8), o


def measure(name, nbytes, host_map):
    kind, seed = TABLES[name]
    e = mox.Engine(device=0, reserve_bytes=nbytes)
    host = corpus.fill(kind, seed, 0, nbytes)
    d = e.alloc(nbytes)
    e.h2d(d, host)
    del host
    e.run_device(d, nbytes)

    def fetch():
        e.fetch().close()

    b = median_ms(fetch)
    t = e.fetch()
    counts, offs, data = t.arrays()
    n, nb = t.n, int(offs[-1])
    t.close()
    top = median_ms(lambda: e.top_words(10).close())
    res = {"table": name, "corpus_bytes": nbytes, "words": n, "word_bytes": nb, "table_bytes": 16 * n + 8 + nb,
           "fetch_ms": b, "top_words_ms": top, "floor_offsets_bytes": 8 * n, "floor_all_bytes": 8 * n + nb, "q": {}}
    queries = {}
    for q in QS:
        words, qdata, qoffs = make_queries(offs, data, q, seed)
        queries[q] = (words, qdata, qoffs)
        got = {}

        def look():
            got["c"] = e.lookup_packed(qdata, qoffs)

        a = median_ms(look)
        _, _, info = e.lookup_packed(qdata, qoffs, with_index=True, with_info=True)
        lens = set(np.diff(qoffs.astype(np.int64)).tolist())
        tl = np.diff(offs.astype(np.int64))
        hit = np.isin(tl, list(lens)) if max(lens) < 64 else (np.isin(tl, [x for x in lens if x < 64]) | (tl >= 64))
        res["q"][q] = {"lookup_ms": a, "info": info, "query_bytes": int(qoffs[-1]), "counts_sum": int(got["c"].sum(dtype=np.uint64)),
                       "table_words_passing_the_length_filter": int(hit.sum()), "their_bytes": int(tl[hit].sum())}
        print("%-6s n=%d q=%d  (a) lookup %.3f ms (%.3f-%.3f)  (b) fetch %.2f ms  found %d distinct %d  filter passes %d words / %d bytes"
              % (name, n, q, a[0], a[1], a[2], b[0], info["found"], info["distinct"], int(hit.sum()), int(tl[hit].sum())), flush=True)
        res["q"][q]["_counts"] = got["c"]
    # q = 10 on the sorted result: what a binary search per query would have to beat
    e.sort_result()
    _, qdata, qoffs = queries[10]
    s10 = median_ms(lambda: e.lookup_packed(qdata, qoffs))
    res["sorted_q10_lookup_ms"] = s10
    assert np.array_equal(e.lookup_packed(qdata, qoffs), res["q"][10]["_counts"])
    print("%-6s sorted result, q=10: lookup %.3f ms (%.3f-%.3f)" % (name, s10[0], s10[1], s10[2]), flush=True)
    if host_map:
        # (c): one fetch, one dict over every word, then the lookups (the dict does not depend on q)
        t0 = time.perf_counter()
        t = e.fetch()
        counts, offs, data = t.arrays()
        t.close()
        t1 = time.perf_counter()
        ol = offs.tolist()
        table = dict(zip((data[x:y] for x, y in zip(ol, ol[1:])), counts.tolist()))
        del ol
        t2 = time.perf_counter()
        res["host_map"] = {"fetch_ms": (t1 - t0) * 1e3, "dict_build_ms": (t2 - t1) * 1e3}
        for q in QS:
            words = queries[q][0]
            t3 = time.perf_counter()
            want = [table.get(w, 0) for w in words]
            t4 = time.perf_counter()
            assert np.array_equal(np.array(want, dtype=np.uint64), res["q"][q]["_counts"]), "lookup differs from the host dict"
            c_ms = (t2 - t0) * 1e3 + (t4 - t3) * 1e3
            res["q"][q]["fetch_dict_lookup_ms"] = c_ms
            print("%-6s q=%d  (c) fetch %.1f + dict %.1f + lookups %.3f = %.1f ms (one run; counts equal (a)'s)"
                  % (name, q, (t1 - t0) * 1e3, (t2 - t1) * 1e3, (t4 - t3) * 1e3, c_ms), flush=True)
        del table
    for q in QS:
        del res["q"][q]["_counts"]
    e.free(d)
    e.close()
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    args = sys.argv[1:]
    nbytes = int(args.pop(0)) if args and args[0].isdigit() else 1 << 30
    host_map = "nomap" not in args
    names = [a for a in args if a != "nomap"] or ["zipf", "hicard"]
    for name in names:
        measure(name, nbytes, host_map)
