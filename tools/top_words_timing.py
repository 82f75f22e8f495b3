"""Device top-k against the fetch it replaces: on the table of
one pass over a corpus in HBM, the median wall time of

  (a) Engine.top_words(10)                  -- selection on the GPU, ten words cross PCIe
  (b) Engine.fetch()                        -- the whole table to the host
  (c) fetch() + mox_print_top_words(t, 10)  -- the only way to the answer without (a)

over REPS repetitions after WARMUP warm-ups, for C2's corpus (1 GiB ZIPF,
1.44 M words) and 1 GiB of HICARD (tens of millions of words).  (c)'s stdout
goes to /dev/null.  Also printed: the passes over counts[n] the selection makes
(level 0, the levels at or below the largest count's highest bit, the tie
pass), their bytes and the HBM rate they imply.

  python tools/top_words_timing.py [bytes] [zipf|hicard ...]
  rocprofv3 --kernel-trace --stats -d DIR -- python tools/top_words_timing.py   (per-kernel times)
"""
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "map-oxidize_amd"))
import mox  # noqa: E402
from mox import corpus  # noqa: E402

REPS, WARMUP, K = 10, 2, 10
TABLES = {"zipf": (corpus.ZIPF, corpus.CONFIGS["C2"]["seed"]), "hicard": (corpus.HICARD, corpus.CONFIGS["C4"]["seed"])}


def median_ms(fn):
    for _ in range(WARMUP):
        fn()
    ts = []
    for _ in range(REPS):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), min(ts), max(ts)


def measure(name, nbytes):
    kind, seed = TABLES[name]
    e = mox.Engine(device=0, reserve_bytes=nbytes)
    host = corpus.fill(kind, seed, 0, nbytes)
    d = e.alloc(nbytes)
    e.h2d(d, host)
    del host
    e.run_device(d, nbytes)
    L = e._L

    def top():
        e.top_words(K).close()

    def fetch():
        e.fetch().close()

    def fetch_print():
        t = e.fetch()
        L.mox_print_top_words(t._p, K)
        t.close()

    a = median_ms(top)
    b = median_ms(fetch)
    # (c) prints through C stdio: fd 1 points at /dev/null while it is timed
    libc = ctypes.CDLL(None)
    sys.stdout.flush()
    saved, null = os.dup(1), os.open(os.devnull, os.O_WRONLY)
    os.dup2(null, 1)
    try:
        c = median_ms(fetch_print)
        libc.fflush(None)
    finally:
        os.dup2(saved, 1)
        os.close(saved)
        os.close(null)
    t = e.fetch()
    counts, offs, _ = t.arrays()
    n, table_bytes, cmax = t.n, 16 * t.n + 8 + int(offs[-1]), int(counts.max()) if t.n else 0
    t.close()
    tw = e.top_words(K)
    words = [(w.decode("utf-8", "replace"), c) for w, c in tw.items()]
    tw.close()
    e.free(d)
    e.close()
    # passes over counts[n]: level 0 always; level l >= 1 (digit bits 56 - 8 l ..) only if a count reaches that digit
    levels = 1 + sum(1 for l in range(1, 8) if cmax >> (56 - 8 * l))
    passes = levels + 1  # + the tie / candidate pass
    res = {
        "table": name, "corpus_bytes": nbytes, "words": n, "table_bytes": table_bytes, "max_count": cmax,
        "top_words_ms": a, "fetch_ms": b, "fetch_print_ms": c,
        "select_levels_run": levels, "select_passes": passes, "select_bytes": passes * 8 * n,
        "select_gbps_if_all_of_a": passes * 8 * n / (a[0] * 1e-3) / 1e9 if n else 0.0,
        "top": words,
    }
    print(json.dumps(res), flush=True)
    print("%-6s n=%d  (a) top_words %.3f ms  (b) fetch %.2f ms  (c) fetch+print %.2f ms  | %d passes x 8n = %.1f MB"
          % (name, n, a[0], b[0], c[0], passes, passes * 8 * n / 1e6), flush=True)


if __name__ == "__main__":
    args = sys.argv[1:]
    nbytes = int(args.pop(0)) if args and args[0].isdigit() else 1 << 30
    for name in (args or ["zipf", "hicard"]):
        measure(name, nbytes)
