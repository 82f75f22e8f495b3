"""Device re-keying against the only way to the same result without it
(DESIGN.md §8): on the table of one pass over a corpus in HBM, the wall time of

  (a) Engine.rekey_result(...)   -- the trimmed table becomes the resident result
  (b) Engine.fetch() + the same strip on the host + reduce_pairs of the
      windowed rows (mox_reduce_pairs on numpy arrays, no Python lists), which
      puts the trimmed table back on the device

on the same engine and table, for punct=True on the ZIPF and HICARD tables
and, as HICARD's words are [a-z0-9] alone (punct=True changes no row there:
the no-op path), for trim=b"0123456789" on HICARD ("hicard-digits"), which
changes about half of its rows.  A re-key replaces the result, so every timed
call is preceded by an untimed pass over the corpus that restores it; (a) and
(b) alternate, REPS times (REPS_BIG on a large table) after WARMUP warm-ups of
each, and every repetition is printed.  The host strip is numpy over the
fetched arrays: the leading and trailing runs of the set's bytes are
counted one byte per step for all rows at once, the windows are gathered into
a packed byte array, empty ones dropped.  (a)'s table is compared with (b)'s in
the same process (as dictionaries, or by words, bytes and tokens on a table of
more than HOST_DICT_MAX words).

  python tools/rekey_timing.py [bytes] [zipf|hicard|hicard-digits ...] [noalt]
  rocprofv3 --kernel-trace --stats -d DIR -- python tools/rekey_timing.py BYTES zipf hicard noalt   (per-kernel times)
"""
import ctypes
import json
import os
import statistics
import string
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "map-oxidize_amd"))
import mox  # noqa: E402
from mox import corpus  # noqa: E402

REPS, WARMUP = 5, 1
REPS_BIG = 3  # repetitions on a table of more than HOST_DICT_MAX words ((b) takes seconds there)
HOST_DICT_MAX = 4 << 20
TABLES = {"zipf": (corpus.ZIPF, corpus.CONFIGS["C2"]["seed"], dict(punct=True)),
          "hicard": (corpus.HICARD, corpus.CONFIGS["C4"]["seed"], dict(punct=True)),
          "hicard-digits": (corpus.HICARD, corpus.CONFIGS["C4"]["seed"], dict(trim=b"0123456789"))}


def strip_set(spec):
    """The spec's bytes as a 256-entry boolean table."""
    t = np.zeros(256, dtype=bool)
    t[list(spec.get("trim", b"") + (string.punctuation.encode() if spec.get("punct") else b""))] = True
    return t


def stat(ts):
    return statistics.median(ts), min(ts), max(ts)


def host_windows(counts, offs, data, IS_PUNCT):
    """(bytes, offs, counts, rows changed) of the rows with the bytes of the set stripped from both ends, empty windows dropped."""
    buf = np.frombuffer(data, dtype=np.uint8)
    o = offs[:-1].astype(np.int64)
    e = offs[1:].astype(np.int64)
    s = o.copy()
    live = np.nonzero(s < e)[0]
    while live.size:  # one leading byte per step, over the rows still being stripped
        live = live[IS_PUNCT[buf[s[live]]]]
        s[live] += 1
        live = live[s[live] < e[live]]
    live = np.nonzero(e > s)[0]
    while live.size:
        live = live[IS_PUNCT[buf[e[live] - 1]]]
        e[live] -= 1
        live = live[e[live] > s[live]]
    lens = e - s
    changed = int((lens != (offs[1:].astype(np.int64) - o)).sum())
    keep = lens > 0
    lens, src = lens[keep], s[keep]
    new_offs = np.zeros(lens.size + 1, dtype=np.uint64)
    np.cumsum(lens, out=new_offs[1:])
    idx = np.repeat(src - new_offs[:-1].astype(np.int64), lens) + np.arange(int(new_offs[-1]), dtype=np.int64)
    return buf[idx], new_offs, np.ascontiguousarray(counts[keep]), changed


def measure(name, nbytes, alt):
    kind, seed, spec = TABLES[name]
    strip = strip_set(spec)
    e = mox.Engine(device=0, reserve_bytes=nbytes)
    host = corpus.fill(kind, seed, 0, nbytes)
    d = e.alloc(nbytes)
    e.h2d(d, host)
    del host

    def restore():
        e.run_device(d, nbytes)

    def rekey():
        restore()
        t0 = time.perf_counter()
        info = e.rekey_result(**spec)
        return (time.perf_counter() - t0) * 1e3, info

    def host_path():
        restore()
        t0 = time.perf_counter()
        t = e.fetch()
        counts, offs, data = t.arrays()
        t1 = time.perf_counter()
        kb, ko, kc, changed = host_windows(counts, offs, data, strip)
        t2 = time.perf_counter()
        e._c(e._L.mox_reduce_pairs(e._h, ctypes.c_void_p(kb.ctypes.data if kb.size else None), ctypes.c_void_p(ko.ctypes.data),
                                   ctypes.c_void_p(kc.ctypes.data), kc.size))
        t3 = time.perf_counter()
        t.close()
        return {"total": (t3 - t0) * 1e3, "fetch": (t1 - t0) * 1e3, "strip": (t2 - t1) * 1e3, "reduce_pairs": (t3 - t2) * 1e3,
                "changed": changed}

    def resident():
        t = e.fetch()
        try:
            return t.as_dict() if t.n <= HOST_DICT_MAX else (t.n, t.tokens, int(t.arrays()[1][-1]))
        finally:
            t.close()

    for _ in range(WARMUP):
        rekey()
        if alt:
            host_path()
    a, b, parts, info = [], [], [], None
    n = None
    for rep in range(REPS_BIG if kind == corpus.HICARD and nbytes > (64 << 20) else REPS):  # interleaved: (a), (b), (a), (b), ...
        ms, info = rekey()
        a.append(ms)
        n = info["words_in"]
        line = "%-13s rep %d (a) rekey %.3f ms" % (name, rep, ms)
        if alt:
            h = host_path()
            b.append(h["total"])
            parts.append(h)
            line += "  (b) fetch %.1f + strip %.1f + reduce_pairs %.1f = %.1f ms" % (h["fetch"], h["strip"], h["reduce_pairs"], h["total"])
        print(line, flush=True)
    res = {"table": name, "corpus_bytes": nbytes, "info": {k: v for k, v in info.items() if k != "ms"},
           "changed_share": info["words_changed"] / max(1, info["words_in"]), "rekey_ms": stat(a), "rekey_ms_all": a}
    line = "%-13s words %d -> %d, changed %d (%.1f %%), dropped %d;  (a) rekey %.3f ms (%.3f-%.3f)" % (
        name, info["words_in"], info["words_out"], info["words_changed"], 100 * res["changed_share"], info["words_dropped"], *stat(a))
    if alt:
        med = {k: statistics.median(p[k] for p in parts) for k in ("fetch", "strip", "reduce_pairs")}
        res.update({"host_ms": stat(b), "host_ms_all": b, "host_parts_median_ms": med})
        line += "  (b) fetch %.1f + strip %.1f + reduce_pairs %.1f = %.1f ms (%.1f-%.1f)  (b)/(a) %.1fx" % (
            med["fetch"], med["strip"], med["reduce_pairs"], *stat(b), stat(b)[0] / stat(a)[0])
        assert parts[-1]["changed"] == info["words_changed"], "the host strip changes other rows"
        want = resident()  # (b)'s, left by the last host_path
        rekey()
        assert resident() == want, "the re-keyed table differs from the host path's"
        line += "  tables equal" if n <= HOST_DICT_MAX else "  words, bytes and tokens equal"
    print(line, flush=True)
    e.free(d)
    e.close()
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    args = sys.argv[1:]
    nbytes = int(args.pop(0)) if args and args[0].isdigit() else 1 << 30
    alt = "noalt" not in args
    names = [x for x in args if x != "noalt"] or ["zipf", "hicard", "hicard-digits"]
    for name in names:
        measure(name, nbytes, alt)
