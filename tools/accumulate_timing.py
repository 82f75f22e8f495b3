"""The device-resident accumulator against what it replaces: a
corpus of `bytes` in HBM, cut into WINDOWS windows at whitespace, counted three
ways, wall time from the first pass to the total being available:

  (a) WINDOWS x (run_range + accumulate)     -- the total stays on the device
  (b) one pass over the whole corpus         -- the floor (a) pays its merges against
  (c) WINDOWS x (run_range + fetch) + a host merge: numpy.unique over the
      windows' words as fixed-width keys, counts summed with numpy.add.at --
      what the parent commit offers (Table.as_dict's Python dict is slower still)

for C2's corpus (1 GiB ZIPF) and 1 GiB of HICARD.  Per merge of (a): its wall
time, the rows of both sources, and the bytes the packer must move (16 n + word
bytes in; 24 per short word + 32 + padded bytes per long word out).  The three
totals are compared in this process: (a) and (b) as fetched arrays (same engine
order expected for words of at most 16 bytes) and, both sorted on the device,
row by row; (c) against the device-sorted (b).

  python tools/accumulate_timing.py [bytes] [zipf|hicard ...] [--no-host]
  rocprofv3 --kernel-trace --stats -d DIR -- python tools/accumulate_timing.py ... --no-host   (per-kernel times)
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "map-oxidize_amd"))
import mox  # noqa: E402
from mox import corpus  # noqa: E402

WINDOWS = 8
TABLES = {"zipf": (corpus.ZIPF, corpus.CONFIGS["C2"]["seed"]), "hicard": (corpus.HICARD, corpus.CONFIGS["C4"]["seed"])}
WS = (9, 10, 11, 12, 13, 32)


def cuts_of(host, k):
    cuts = [0]
    for j in range(1, k):
        p = max(cuts[-1], len(host) * j // k)
        while p < len(host) and host[p - 1] not in WS:
            p += 1
        cuts.append(p)
    cuts.append(len(host))
    return cuts


def keys_of(counts, offs, raw, width):
    """The table's words as a fixed-width 'S' array (zero padded)."""
    offs = offs.astype(np.int64)
    lens = np.diff(offs)
    buf = np.frombuffer(raw, np.uint8)
    out = np.zeros((counts.size, width), np.uint8)
    rows = np.repeat(np.arange(counts.size), lens)
    cols = np.arange(int(offs[-1])) - np.repeat(offs[:-1], lens)
    out[rows, cols] = buf
    return out.view("S%d" % width).ravel()


def measure(name, nbytes, host_merge):
    kind, seed = TABLES[name]
    e = mox.Engine(device=0, reserve_bytes=nbytes)
    host = corpus.fill(kind, seed, 0, nbytes)
    cuts = cuts_of(host, WINDOWS)
    d = e.alloc(nbytes)
    e.h2d(d, host)
    del host
    wins = list(zip(cuts, cuts[1:]))

    def run_a():
        e.accumulate_reset()
        merges = []
        t0 = time.perf_counter()
        for lo, hi in wins:
            e.run_range(d, nbytes, lo, hi, True)
            n_run, n_tot = e.stats()["uniques"], e.accumulate_info()["words"]
            t1 = time.perf_counter()
            e.accumulate()
            merges.append({"ms": (time.perf_counter() - t1) * 1e3, "rows_total": n_tot, "rows_run": n_run,
                           "rows_after": e.accumulate_info()["words"]})
        return (time.perf_counter() - t0) * 1e3, merges

    def run_b():
        t0 = time.perf_counter()
        e.run_device(d, nbytes)
        return (time.perf_counter() - t0) * 1e3

    def fetched():
        t = e.fetch()
        try:
            return t.arrays(), t.n, t.tokens
        finally:
            t.close()

    def same(x, y):
        return all(np.array_equal(p, q) for p, q in zip(x[:2], y[:2])) and x[2] == y[2]

    run_a()  # warm-up: buffers grown
    a_ms, merges = run_a()
    A, _, a_tok = fetched()
    e.sort_result()  # the total, sorted on the device: comparable row by row
    As = fetched()[0]
    run_b()
    b_ms = min(run_b() for _ in range(3))
    B, n, tokens = fetched()
    nb = int(B[1][-1]) if n else 0
    same_order = same(A, B)
    lens = np.diff(B[1].astype(np.int64))
    width = int(lens.max()) if n else 1
    n_short = int((lens <= 16).sum())
    del A, B, lens
    e.sort_result()
    Bs = fetched()[0]
    equal_ab = same(As, Bs) and a_tok == tokens
    del As
    kb = keys_of(*Bs, width) if host_merge else None
    res = {"table": name, "corpus_bytes": nbytes, "windows": WINDOWS, "words": n, "tokens": tokens, "table_bytes": 16 * n + 8 + nb,
           "a_windows_accumulate_ms": a_ms, "b_one_pass_ms": b_ms, "a_over_b": a_ms / b_ms,
           "a_merge_ms_sum": sum(m["ms"] for m in merges), "merges": merges,
           "a_equals_b": bool(equal_ab), "a_same_engine_order_as_b": bool(same_order),
           # packer traffic of the last merge at the final sizes: both sources in, wire image out
           "last_merge_in_bytes": 16 * (merges[-1]["rows_total"] + merges[-1]["rows_run"]),
           "final_short_words": n_short, "final_word_bytes": nb}
    if host_merge:
        t0 = time.perf_counter()
        ks, cs = [], []
        fetch_ms = 0.0
        for lo, hi in wins:
            e.run_range(d, nbytes, lo, hi, True)
            t1 = time.perf_counter()
            t = e.fetch()
            arr = t.arrays()
            t.close()
            fetch_ms += (time.perf_counter() - t1) * 1e3
            ks.append(keys_of(*arr, width))
            cs.append(arr[0])
        keys, inv = np.unique(np.concatenate(ks), return_inverse=True)
        tot = np.zeros(keys.size, np.uint64)
        np.add.at(tot, inv, np.concatenate(cs))
        res["c_windows_fetch_host_merge_ms"] = (time.perf_counter() - t0) * 1e3
        res["c_fetch_part_ms"] = fetch_ms
        res["c_equals_b"] = bool(np.array_equal(keys, kb) and np.array_equal(tot, Bs[0]))
    e.free(d)
    e.close()
    print(json.dumps(res), flush=True)
    print("%-6s n=%d  (a) %d x (run_range + accumulate) %.2f ms (merges %.2f)  (b) one pass %.2f ms  a/b %.2f  %s  a==b %s %s"
          % (name, n, WINDOWS, a_ms, res["a_merge_ms_sum"], b_ms, a_ms / b_ms,
             "(c) fetch + host merge %.1f ms" % res["c_windows_fetch_host_merge_ms"] if host_merge else "",
             equal_ab, "c==b %s" % res["c_equals_b"] if host_merge else ""), flush=True)


if __name__ == "__main__":
    args = sys.argv[1:]
    host_merge = "--no-host" not in args
    args = [a for a in args if a != "--no-host"]
    nbytes = int(args.pop(0)) if args and args[0].isdigit() else 1 << 30
    for name in (args or ["zipf", "hicard"]):
        measure(name, nbytes, host_merge)
