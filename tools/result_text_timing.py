"""Device text rendering against the road it replaces: on the
table of one pass over a corpus in HBM, the median wall time of

  (a) Engine.result_text()                      -- text formatted on the GPU, into host memory
  (a') mox_result_text + mox_text_free          -- (a) without the copy into a Python bytes object
  (b) Engine.write_result(/dev/shm/...)         -- the same, streamed to a file
  (c) Engine.fetch()                            -- the whole table to the host
  (d) fetch() + write_final_result(/dev/shm/..) -- the old road to the file (host formatter)

over REPS repetitions after WARMUP warm-ups, for C2's corpus (1 GiB ZIPF,
1.44 M words) and 1 GiB of HICARD (tens of millions of words).  Also: (b) under
MOX_TEXT_SLICE = 8, 32 and 128 MiB, the host's share of (b) alone (os.pwrite of
the finished text in 32 MiB pieces), and the bytes k_tx_emit reads (16 per word
of counts and offsets + the words) and writes (the text) per call.

  python tools/result_text_timing.py [bytes] [zipf|hicard ...] [--reps N] [--warmup N] [--no-old]
  rocprofv3 --kernel-trace --stats -d DIR -- python tools/result_text_timing.py --no-old   (per-kernel times)
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

REPS, WARMUP = 10, 2
TABLES = {"zipf": (corpus.ZIPF, corpus.CONFIGS["C2"]["seed"]), "hicard": (corpus.HICARD, corpus.CONFIGS["C4"]["seed"])}
SLICES_MIB = (8, 32, 128)
OUT_DIR = "/dev/shm" if os.path.isdir("/dev/shm") else "/tmp"


def median_ms(fn, reps=None, warmup=None):
    for _ in range(WARMUP if warmup is None else warmup):
        fn()
    ts = []
    for _ in range(REPS if reps is None else reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), min(ts), max(ts)


def measure(name, nbytes, old):
    kind, seed = TABLES[name]
    e = mox.Engine(device=0, reserve_bytes=nbytes)
    host = corpus.fill(kind, seed, 0, nbytes)
    d = e.alloc(nbytes)
    e.h2d(d, host)
    del host
    e.run_device(d, nbytes)
    new_path = os.path.join(OUT_DIR, "mox_result_text_new.%d.txt" % os.getpid())
    old_path = os.path.join(OUT_DIR, "mox_result_text_old.%d.txt" % os.getpid())

    def text():
        e.result_text()

    def text_c():
        p, n = ctypes.POINTER(ctypes.c_uint8)(), ctypes.c_uint64()
        e._c(e._L.mox_result_text(e._h, ctypes.byref(p), ctypes.byref(n)))
        e._L.mox_text_free(p)

    def write():
        e.write_result(new_path)

    def fetch():
        e.fetch().close()

    def fetch_write():
        t = e.fetch()
        t.write_final_result(old_path)
        t.close()

    res = {"table": name, "corpus_bytes": nbytes}
    try:
        res["result_text_ms"] = a = median_ms(text)
        res["result_text_c_ms"] = ac = median_ms(text_c)
        res["write_result_ms"] = b = median_ms(write)
        res["fetch_ms"] = c = median_ms(fetch)
        dd = None
        if old:
            res["fetch_write_ms"] = dd = median_ms(fetch_write)
        by_slice = {}
        saved = os.environ.get("MOX_TEXT_SLICE")
        for mib in SLICES_MIB:
            os.environ["MOX_TEXT_SLICE"] = str(mib << 20)
            by_slice[mib] = (median_ms(write), median_ms(text))
        if saved is None:
            del os.environ["MOX_TEXT_SLICE"]
        else:
            os.environ["MOX_TEXT_SLICE"] = saved
        res["write_result_ms_by_slice_mib"] = {k: v[0] for k, v in by_slice.items()}
        res["result_text_ms_by_slice_mib"] = {k: v[1] for k, v in by_slice.items()}
        txt = e.result_text()
        if old:
            with open(old_path, "rb") as f:
                res["same_as_old_writer"] = f.read() == txt
        with open(new_path, "rb") as f:
            res["file_equals_text"] = f.read() == txt

        def host_write():  # the host's share of (b): the finished text to the file in slice-sized pieces
            fd = os.open(new_path, os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o666)
            mv = memoryview(txt)
            for off in range(0, len(txt), 32 << 20):
                os.pwrite(fd, mv[off:off + (32 << 20)], off)
            os.close(fd)

        res["pwrite_only_ms"] = pw = median_ms(host_write)
        t = e.fetch()
        _, offs, _ = t.arrays()
        n, nb = t.n, int(offs[-1])
        t.close()
        res.update(words=n, word_bytes=nb, table_bytes=16 * n + 8 + nb, text_bytes=len(txt),
                   emit_read_bytes=16 * n + nb, emit_write_bytes=len(txt))
    finally:
        for p in (new_path, old_path):
            if os.path.exists(p):
                os.unlink(p)
        e.free(d)
        e.close()
    print(json.dumps(res), flush=True)
    print("%-6s n=%d text %.1f MB (table %.1f MB)  (a) result_text %.2f ms (C call alone %.2f)  (b) write_result %.2f ms  (c) fetch %.2f ms  (d) fetch+write %s ms"
          "  | pwrite alone %.2f ms | (b) by slice MiB: %s"
          % (name, n, len(txt) / 1e6, res["table_bytes"] / 1e6, a[0], ac[0], b[0], c[0], "%.2f" % dd[0] if dd else "-", pw[0],
             ", ".join("%d: %.2f" % (k, v[0][0]) for k, v in by_slice.items())), flush=True)


if __name__ == "__main__":
    args = sys.argv[1:]
    old = True
    if "--no-old" in args:
        args.remove("--no-old")
        old = False
    for flag in ("--reps", "--warmup"):
        if flag in args:
            i = args.index(flag)
            v = int(args[i + 1])
            del args[i:i + 2]
            if flag == "--reps":
                REPS = v
            else:
                WARMUP = v
    nbytes = int(args.pop(0)) if args and args[0].isdigit() else 1 << 30
    for name in (args or ["zipf", "hicard"]):
        measure(name, nbytes, old)
