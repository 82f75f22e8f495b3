"""Device ranking against the only way to the same file without it
(DESIGN.md §8): on the table of one pass over a corpus in HBM, the median wall
time of

  (a) Engine.rank_result() + Engine.write_result(path)
        -- the table is ordered by count and rendered on the GPU; only the
           text crosses PCIe
  (b) Engine.fetch() + a stable host argsort by count + the host writer
        -- the whole table to the host, numpy's stable argsort of the
           complemented counts, the table permuted with numpy (chunked
           gathers, no Python loop over words), mox_write_final_result

over REPS repetitions after WARMUP warm-ups, for C2's corpus (1 GiB ZIPF,
1.44 M words) and 1 GiB of HICARD (91 M words).  A ranking replaces the
result, and ranking a ranked table reads its rows in order, so every timed call
is preceded by an untimed pass over the corpus that restores the engine-order
table.  Once, before the timing, the device's ranked table and file are compared
byte for byte with the host's, both made from one resident table.  Also measured, on the
ranked table: fetch_rows(0, 100000) against a full fetch().  Also printed: the
radix passes the ranking ran, the bytes each moves (keys, row indices and the
per-tile digit counts) and the rate they imply if the whole call were passes.

  python tools/rank_timing.py [bytes] [zipf|hicard ...] [noalt] [reps=N] [warmup=N]
  rocprofv3 --kernel-trace --stats -d DIR -- python tools/rank_timing.py BYTES hicard noalt reps=3   (per-kernel times)
"""
import ctypes
import filecmp
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "map-oxidize_amd"))
import mox  # noqa: E402
from mox import corpus  # noqa: E402

REPS, WARMUP = 10, 2
PAGE = 100000
TILE = 4096            # RK_TILE (mox_rank.hip)
GATHER_CHUNK = 1 << 22  # words per numpy gather of the host permutation
TABLES = {"zipf": (corpus.ZIPF, corpus.CONFIGS["C2"]["seed"]), "hicard": (corpus.HICARD, corpus.CONFIGS["C4"]["seed"])}


def stat(ts):
    return statistics.median(ts), min(ts), max(ts)


def permuted_table(order, counts, offs, data):
    """(counts, offs, bytes) of the table with row r = old row order[r], built with numpy."""
    lens = np.diff(offs.astype(np.int64))[order]
    new_offs = np.zeros(order.size + 1, dtype=np.uint64)
    np.cumsum(lens, out=new_offs[1:])
    src = offs[:-1].astype(np.int64)[order]
    buf = np.frombuffer(data, dtype=np.uint8)
    out = np.empty(int(new_offs[-1]), dtype=np.uint8)
    for lo in range(0, order.size, GATHER_CHUNK):
        hi = min(order.size, lo + GATHER_CHUNK)
        b0, b1 = int(new_offs[lo]), int(new_offs[hi])
        idx = np.repeat(src[lo:hi] - new_offs[lo:hi].astype(np.int64), lens[lo:hi]) + np.arange(b0, b1, dtype=np.int64)
        out[b0:b1] = buf[idx]
    return np.ascontiguousarray(counts[order]), new_offs, out


def measure(name, nbytes, alt, reps, warmup):
    kind, seed = TABLES[name]
    e = mox.Engine(device=0, reserve_bytes=nbytes)
    host = corpus.fill(kind, seed, 0, nbytes)
    d = e.alloc(nbytes)
    e.h2d(d, host)
    del host
    tmp = tempfile.TemporaryDirectory()
    path_a, path_b = os.path.join(tmp.name, "ranked_device.txt"), os.path.join(tmp.name, "ranked_host.txt")

    def restore():
        e.run_device(d, nbytes)

    def device_path():
        restore()
        t0 = time.perf_counter()
        info = e.rank_result()
        t1 = time.perf_counter()
        e.write_result(path_a)
        t2 = time.perf_counter()
        return {"total": (t2 - t0) * 1e3, "rank": (t1 - t0) * 1e3, "write": (t2 - t1) * 1e3}, info

    def host_rank_and_write():
        """The resident table fetched, ranked on the host and written to path_b: (times of the parts, the ranked arrays)."""
        t0 = time.perf_counter()
        t = e.fetch()
        counts, offs, data = t.arrays()
        t1 = time.perf_counter()
        order = np.argsort(~counts, kind="stable")  # complemented u64 counts ascending = counts descending, ties in table order
        t2 = time.perf_counter()
        pc, po, pb = permuted_table(order, counts, offs, data)
        t3 = time.perf_counter()
        tab = mox._Table(pc.size, t.tokens, pc.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)),
                         po.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), pb.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)))
        e._c(e._L.mox_write_final_result(ctypes.byref(tab), path_b.encode()))
        t4 = time.perf_counter()
        t.close()
        return {"total": (t4 - t0) * 1e3, "fetch": (t1 - t0) * 1e3, "argsort": (t2 - t1) * 1e3, "permute": (t3 - t2) * 1e3,
                "write": (t4 - t3) * 1e3}, (pc, po, pb)

    def host_path():
        restore()
        return host_rank_and_write()[0]

    if alt:
        # once, on ONE resident table (the engine order of long words differs from pass to pass, and with it
        # the order of ties): the host's ranking of the fetch, then the device's ranking of the same result
        restore()
        _, (pc, po, pb) = host_rank_and_write()
        e.rank_result()
        t = e.fetch()
        dc, do, dd = t.arrays()
        t.close()
        assert np.array_equal(dc, pc), "ranked counts differ from the host's at row %d" % int(np.argmax(dc != pc))
        assert np.array_equal(do, po), "ranked offsets differ from the host's at row %d" % int(np.argmax(do != po))
        assert dd == pb.tobytes(), "ranked bytes differ from the host's"
        e.write_result(path_a)
        assert filecmp.cmp(path_a, path_b, shallow=False), "the device's ranked file differs from the host's"
        del pc, po, pb, dc, do, dd
    a, b, info = [], [], None
    for k in range(warmup + reps):  # interleaved: (a), (b), (a), (b), ...
        pa, info = device_path()
        if k >= warmup:
            a.append(pa)
        if alt:
            pb_ = host_path()
            if k >= warmup:
                b.append(pb_)
    n, passes = info["words"], info["digit_passes"]
    nt = (n + TILE - 1) // TILE
    # per pass: k_rk_hist reads the keys; k_rk_scatter reads keys (+ row indices after pass 0) and writes both; the
    # (digit, tile) counts are written once, read by the part scan, read and written by the apply scan, read by the scatter
    pass_bytes = [8 * n + (8 * n if k == 0 else 12 * n) + 12 * n + 5 * 1024 * nt for k in range(passes)]
    med_a = {k: statistics.median(p[k] for p in a) for k in ("total", "rank", "write")}
    res = {"table": name, "corpus_bytes": nbytes, "words": n, "max_count": info["max_count"], "digit_passes": passes,
           "device_bytes": info["device_bytes"], "reps": reps, "warmup": warmup,
           "device_ms": stat([p["total"] for p in a]), "device_parts_median_ms": med_a, "device_ms_all": [p["total"] for p in a],
           "rank_ms": stat([p["rank"] for p in a]),
           "pass_bytes": pass_bytes, "passes_gbps_if_all_of_rank": sum(pass_bytes) / (med_a["rank"] * 1e-3) / 1e9 if passes else 0.0}
    line = "%-6s n=%d  (a) rank %.2f + write %.1f = %.1f ms (%.1f-%.1f)  | %d passes, the last moves %.1f MB" % (
        name, n, med_a["rank"], med_a["write"], *stat([p["total"] for p in a]), passes, (pass_bytes[-1] if passes else 0) / 1e6)
    if alt:
        med_b = {k: statistics.median(p[k] for p in b) for k in ("total", "fetch", "argsort", "permute", "write")}
        res.update({"host_ms": stat([p["total"] for p in b]), "host_parts_median_ms": med_b, "host_ms_all": [p["total"] for p in b]})
        line += "  (b) fetch %.1f + argsort %.1f + permute %.1f + write %.1f = %.1f ms  (b)/(a) %.1fx  files equal" % (
            med_b["fetch"], med_b["argsort"], med_b["permute"], med_b["write"], med_b["total"], med_b["total"] / med_a["total"])
    else:
        line += "  (b) not measured"
    print(line, flush=True)

    # a page of the ranked table against the whole table (the result is ranked: the last device_path left it so)
    def timed(fn):
        for _ in range(warmup):
            fn()
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            fn()
            ts.append((time.perf_counter() - t0) * 1e3)
        return stat(ts)

    res["fetch_rows_ms"] = timed(lambda: e.fetch_rows(0, PAGE).close())
    res["fetch_ms"] = timed(lambda: e.fetch().close())
    res["page_rows"] = min(PAGE, n)
    print("%-6s n=%d  fetch_rows(0, %d) %.3f ms  fetch() %.2f ms" % (name, n, PAGE, res["fetch_rows_ms"][0], res["fetch_ms"][0]), flush=True)
    print(json.dumps(res), flush=True)
    e.free(d)
    e.close()
    tmp.cleanup()


if __name__ == "__main__":
    args = sys.argv[1:]
    nbytes = int(args.pop(0)) if args and args[0].isdigit() else 1 << 30
    opts = dict(a.split("=") for a in args if "=" in a)
    names = [a for a in args if a in TABLES] or ["zipf", "hicard"]
    for name in names:
        measure(name, nbytes, "noalt" not in args, int(opts.get("reps", REPS)), int(opts.get("warmup", WARMUP)))
