"""Device histograms against the only way to the same bins without them
(DESIGN.md §8): on the table of one pass over a corpus in HBM, per key the
median wall time of

  (a) Engine.histogram(key)
        -- keys, sort and run-length on the GPU; 4 x bins numbers cross PCIe
  (b) Engine.fetch() + the host histogram
        -- the whole table to the host, then numpy: np.unique(counts,
           return_counts=True) for "count", the same over the word lengths for
           "bytes", over the lengths minus the continuation bytes (one
           np.add.reduceat over the word bytes) for "chars", over the packed first window (four
           gathers of one byte per word) for "first"; np.add.at for the tokens
           per bin is NOT included: (b) computes words per bin only

for C2's corpus (1 GiB ZIPF, 1.44 M words) and 1 GiB of HICARD (91 M words).
The histogram only reads, so one resident table serves every call.  Before the
timing, each key's device bins (keys and words) are compared with the host's.
Then histogram("count") against rank_result() on the same table: the same sort,
without the ranking's materialising passes; a ranking replaces the result, so an
untimed pass restores the engine-order table before each of its timed calls.
(a) runs REPS times after WARMUP warm-ups, (b) HOST_REPS times after one.

  python tools/hist_timing.py [bytes] [zipf|hicard ...] [noalt] [reps=N] [warmup=N] [hreps=N]
  rocprofv3 --kernel-trace --stats -d DIR -- python tools/hist_timing.py BYTES hicard noalt reps=3   (per-kernel times)
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

REPS, WARMUP, HOST_REPS = 10, 2, 3
KEYS = ("count", "bytes", "chars", "first")
TABLES = {"zipf": (corpus.ZIPF, corpus.CONFIGS["C2"]["seed"]), "hicard": (corpus.HICARD, corpus.CONFIGS["C4"]["seed"])}


def stat(ts):
    return statistics.median(ts), min(ts), max(ts)


def host_keys(key, counts, offs, data):
    """The key of every row, with numpy (no Python loop over words)."""
    if key == "count":
        return counts
    lens = np.diff(offs)
    if key == "bytes":
        return lens
    buf = np.frombuffer(data, dtype=np.uint8)
    if key == "chars":
        cont = ((buf & 0xC0) == 0x80).view(np.uint8)
        return lens - np.add.reduceat(cont, offs[:-1].astype(np.int64), dtype=np.uint64)  # (no word is empty)
    # first: the first byte and the continuation bytes behind it, at most 4, big-endian in bits 39..8, the length in bits 7..0
    o = offs[:-1].astype(np.int64)
    out = buf[np.minimum(o, buf.size - 1)].astype(np.uint64) << np.uint64(32)
    wl = np.ones(o.size, dtype=np.uint64)
    more = lens > 0
    for j in (1, 2, 3):
        b = buf[np.minimum(o + j, buf.size - 1)]
        more = more & (lens > j) & ((b & 0xC0) == 0x80)
        out |= np.where(more, b.astype(np.uint64) << np.uint64(32 - 8 * j), np.uint64(0))
        wl += more.astype(np.uint64)
    return np.where(lens > 0, out | wl, np.uint64(0))


def measure(name, nbytes, alt, reps, warmup, hreps):
    kind, seed = TABLES[name]
    e = mox.Engine(device=0, reserve_bytes=nbytes)
    host = corpus.fill(kind, seed, 0, nbytes)
    d = e.alloc(nbytes)
    e.h2d(d, host)
    del host
    e.run_device(d, nbytes)
    res = {"table": name, "corpus_bytes": nbytes, "reps": reps, "warmup": warmup, "host_reps": hreps, "keys": {}}

    def host_path(key):
        t0 = time.perf_counter()
        t = e.fetch()
        counts, offs, data = t.arrays()
        t1 = time.perf_counter()
        k, w = np.unique(host_keys(key, counts, offs, data), return_counts=True)
        t2 = time.perf_counter()
        t.close()
        return {"total": (t2 - t0) * 1e3, "fetch": (t1 - t0) * 1e3, "hist": (t2 - t1) * 1e3}, (k, w)

    for key in KEYS:
        a, info = [], None
        for k in range(warmup + reps):
            t0 = time.perf_counter()
            h = e.histogram(key, with_info=True)
            ms = (time.perf_counter() - t0) * 1e3
            info = h[6]
            if k >= warmup:
                a.append(ms)
        row = {"words": info["words"], "bins": info["bins"], "max_key": info["max_key"], "digit_passes": info["digit_passes"],
               "device_bytes": info["device_bytes"], "device_ms": stat(a), "device_ms_all": a}
        line = "%-6s %-5s n=%d bins=%d passes=%d  (a) histogram %.3f ms (%.3f-%.3f)" % (
            name, key, info["words"], info["bins"], info["digit_passes"], *stat(a))
        if alt:
            b = []
            for k in range(1 + hreps):
                p, (hk, hw) = host_path(key)
                if k == 0:
                    assert np.array_equal(h[0], hk.astype(np.uint64)), "%s: the device's keys differ from the host's" % key
                    assert np.array_equal(h[1], hw.astype(np.uint64)), "%s: the device's words per bin differ from the host's" % key
                else:
                    b.append(p)
            med = {k: statistics.median(p[k] for p in b) for k in ("total", "fetch", "hist")}
            row.update({"host_ms": stat([p["total"] for p in b]), "host_parts_median_ms": med, "host_over_device": med["total"] / stat(a)[0]})
            line += "  (b) fetch %.1f + host %.1f = %.1f ms  (b)/(a) %.1fx  bins equal" % (med["fetch"], med["hist"], med["total"],
                                                                                           med["total"] / stat(a)[0])
        else:
            line += "  (b) not measured"
        res["keys"][key] = row
        print(line, flush=True)

    # the same sort with the ranking's materialising passes behind it
    ranks = []
    for k in range(warmup + reps):
        e.run_device(d, nbytes)  # untimed: the engine-order table again
        t0 = time.perf_counter()
        e.rank_result()
        if k >= warmup:
            ranks.append((time.perf_counter() - t0) * 1e3)
    res["rank_ms"] = stat(ranks)
    res["rank_over_hist_count"] = stat(ranks)[0] / res["keys"]["count"]["device_ms"][0]
    print("%-6s rank_result %.3f ms (%.3f-%.3f)  = %.2fx histogram(count)" % (name, *stat(ranks), res["rank_over_hist_count"]), flush=True)
    print(json.dumps(res), flush=True)
    e.free(d)
    e.close()


if __name__ == "__main__":
    args = sys.argv[1:]
    nbytes = int(args.pop(0)) if args and args[0].isdigit() else 1 << 30
    opts = dict(a.split("=") for a in args if "=" in a)
    names = [a for a in args if a in TABLES] or ["zipf", "hicard"]
    for name in names:
        measure(name, nbytes, "noalt" not in args, int(opts.get("reps", REPS)), int(opts.get("warmup", WARMUP)),
                int(opts.get("hreps", HOST_REPS)))
