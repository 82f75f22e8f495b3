"""GPU: the device bytewise sort (map-oxidize_amd/csrc/mox_bsort.hip) on the
tables of bsort_cases.py, each built to land on one edge of its kernels (the
CPU tests in test_bsort_model.py assert that geometry).  Every test gives an
engine with MOX_F_SORT_BYTES a shuffled table through mox_reduce_pairs and
compares the fetched list word for word and count for count with Python's
sorted() over bytes (Rust String Ord): exact, no tolerance.

Both sort modes run: the default one (the first tie levels without a host
round trip; a run past RUN_LMAX makes it give up and run again checked) and
MOX_BSORT_CHECKED (every level read back; a subset with such a run is
radix-sorted with the run id as the top digits).  With MOX_VERBOSE the sort
prints one `bsort:` line per attempt on stderr, which tells the modes apart.

Test -> what it reaches in mox_bsort.hip <- the CPU assertion that guarantees it:
  sizes_on_wave_and_tile_edges -> the carve-up and its alignment check at odd n, partial waves /
      tiles of k_os_pass, k_bs_out2's last block without a whole 16-byte line <- test_case_sizes
  run_geometry -> k_bs_segsort (SEG_MAX overhang, prev_run, cut, listing), k_bs_longsort at
      RUN_LMAX, the -1 give-up at RUN_LMAX + 1 <- test_case_run_geometry, test_case_run_geometry_over
  checked_radix_run_id_digits -> digit_of(d >= 8), radix_sort(zeroed = false) on 10 and 11
      digits <- test_case_run_digits (nrb_of)
  output_stage_boundaries -> k_bs_out2 staged / unstaged at OUT_STAGE and OUT_STAGE + 1, unstaged
      in-key and table words <- test_case_out_stage
  deep_ties_and_buffer_end -> levels past EAGER_LEVELS, the lvt / rbs rings, window() at the end
      of the byte buffer <- test_case_deep_ties
  counts_keep_64_bits -> BPay.count, k_bs_out1;  word_of_16_mib -> err & 4 and the host sort
  engine_reuse_large_then_small -> every array of s_tmp found stale
  one_region_forced, borrowed_pass_buffers -> the reused status region and the borrowed slabs of
      bsort_once <- the sort's own MOX_VERBOSE line

Not covered: 4 run-id digits (2^24 tie runs, ~33 M words: no seconds-long
test), and a word of 2^24 - 1 bytes staying on the device (see
test_word_of_16_mib_sorts_on_the_host)."""
import os
import random
import re
import subprocess
import sys

import pytest

import bsort_cases as C
import mox
from conftest import ROOT

pytestmark = pytest.mark.gpu

MODES = pytest.mark.parametrize("checked", [False, True], ids=["eager", "checked"])


def set_mode(monkeypatch, checked):
    if checked:
        monkeypatch.setenv("MOX_BSORT_CHECKED", "1")
    else:
        monkeypatch.delenv("MOX_BSORT_CHECKED", raising=False)


def engine():
    return mox.Engine(device=0, flags=mox.MOX_F_SORT_BYTES)


def assert_sorts(e, words, counts=None):
    """reduce_pairs(words, counts) on engine e is sorted(zip(words, counts))."""
    if counts is None:
        counts = list(range(1, len(words) + 1))
    t = e.reduce_pairs(words, counts)
    try:
        got = list(t.items())
    finally:
        t.close()
    want = sorted(zip(words, counts))
    assert len(got) == len(want)
    if got != want:
        j = next(i for i, (g, w) in enumerate(zip(got, want)) if g != w)
        raise AssertionError("sorted table differs first at %d of %d: got %r, want %r" % (j, len(want), got[j], want[j]))


def bsort_lines(err):
    """The sort's MOX_VERBOSE lines as dicts of ints (borrowed: (K, M))."""
    out = []
    for m in re.finditer(r"^bsort: n=(\d+) checked=(\d) one_region=(\d) borrowed=(\d+)/(\d+)$", err, re.M):
        n, c, o, k, tot = map(int, m.groups())
        out.append({"n": n, "checked": c, "one_region": o, "borrowed": (k, tot)})
    return out


@MODES
def test_sizes_on_wave_and_tile_edges(monkeypatch, checked):
    """Tables of 2 .. 2 tiles + 1 words on the wave (64), block (256) and tile
    (4,096) edges, odd sizes among them (the scratch carve-up follows n: the
    shapes of the round-6 fault in k_bs_ghist), bytes 0x00 / 0x7f / 0x80 / 0xff
    in the words.  A fresh engine per size: no scratch of a bigger table below."""
    set_mode(monkeypatch, checked)
    for n in C.SIZE_NS:
        e = engine()
        try:
            assert_sorts(e, C.sizes(n))
        finally:
            e.close()


@MODES
def test_run_geometry(monkeypatch, capfd, checked):
    """Tie runs of exactly SEG_MAX and SEG_MAX + 1 records around the first
    SEG_CH boundary of level 1's subset, a run across the second boundary and
    one of exactly RUN_LMAX (k_bs_segsort's window, prev_run and cut logic,
    k_bs_longsort's full LDS): the default mode finishes on its own.  With
    RUN_LMAX + 1 it gives up and the checked mode's radix sorts the subset."""
    set_mode(monkeypatch, checked)
    monkeypatch.setenv("MOX_VERBOSE", "1")
    for words, modes in ((C.run_geometry(), [0]), (C.run_geometry_over(), [0, 1])):
        e = engine()
        try:
            capfd.readouterr()
            assert_sorts(e, words)
            lines = bsort_lines(capfd.readouterr().err)
        finally:
            e.close()
        assert [ln["checked"] for ln in lines] == ([1] if checked else modes)
        assert all(ln["n"] == len(words) and ln["one_region"] == 0 and ln["borrowed"][0] == 0 for ln in lines)


@MODES
@pytest.mark.parametrize("pairs", [300, 70_000])
def test_checked_radix_run_id_digits(monkeypatch, capfd, pairs, checked):
    """The checked mode's radix over a tie subset sorts on 8 key digits plus
    the bytes of the run ids: 302 run ids (2 digits: digit 9) and 70,002
    (3 digits: digit 10, and the memset of 11 digits' status regions).  The
    default mode gets there through its give-up and re-run (a run of 5,000).
    4 digits would need 2^24 runs (~33 M words) and are left out."""
    set_mode(monkeypatch, checked)
    monkeypatch.setenv("MOX_VERBOSE", "1")
    words = C.run_digits(pairs)
    e = engine()
    try:
        capfd.readouterr()
        assert_sorts(e, words)
        lines = bsort_lines(capfd.readouterr().err)
    finally:
        e.close()
    assert [ln["checked"] for ln in lines] == ([1] if checked else [0, 1])


@MODES
def test_output_stage_boundaries(monkeypatch, checked):
    """k_bs_out2: a block of exactly OUT_STAGE bytes (staged), of OUT_STAGE + 1
    (byte by byte), and a table whose blocks are staged in-key words, unstaged
    in-key + table words, unstaged table words and a last block of one word."""
    set_mode(monkeypatch, checked)
    for words in C.out_stage():
        e = engine()
        try:
            assert_sorts(e, words)
        finally:
            e.close()


@MODES
def test_deep_ties_and_buffer_end(monkeypatch, checked):
    """Proper-prefix pairs on the window edges (7|8, 8|9, 14|15, 21|22, 22|23
    bytes) and words tied through five levels (the lvt / rbs rings wrap; past
    EAGER_LEVELS the default mode reads back level by level).  The reduce lays
    words longer than 16 bytes out last and every such word here is in a tie
    run at level 2 or deeper, so whichever ends the byte buffer reads its last
    windows into the buffer's 64 bytes of slack."""
    set_mode(monkeypatch, checked)
    e = engine()
    try:
        assert_sorts(e, C.deep_ties())
    finally:
        e.close()


@MODES
def test_counts_keep_64_bits(monkeypatch, checked):
    """Counts of 2^32 and more come through BPay and k_bs_out1 whole."""
    set_mode(monkeypatch, checked)
    words = C.sizes(257)
    rng = random.Random(64)
    edge = [1, (1 << 32) - 1, 1 << 32, 1 << 63, (1 << 64) - 1]
    counts = [edge[i % len(edge)] if i % 2 else rng.getrandbits(64) | 1 for i in range(len(words))]
    assert set(edge) <= set(counts)
    e = engine()
    try:
        assert_sorts(e, words, counts)
    finally:
        e.close()


@MODES
def test_engine_reuse_large_then_small(monkeypatch, checked):
    """One engine: a table that goes through the checked radix, then 3 words,
    then two tiles + 1, then a run past RUN_LMAX again; each sort finds the
    scratch (status words, histograms, flags, run list) of the one before."""
    set_mode(monkeypatch, checked)
    e = engine()
    try:
        assert_sorts(e, C.run_digits(300))
        assert_sorts(e, [b"b", b"a\xff", b"a"], [7, 8, 9])
        assert_sorts(e, C.sizes(2 * C.OS_TILE + 1))
        assert_sorts(e, C.run_geometry_over())
    finally:
        e.close()


@MODES
def test_word_of_16_mib_sorts_on_the_host(monkeypatch, checked):
    """A word of exactly 2^24 bytes does not fit BPay's 24-bit length: k_bs_init
    flags it (err & 4), the device sort reports it and mox_fetch_table sorts
    the table on the host instead.  (A word of 2^24 - 1 bytes stays on the
    device, where k_bs_out2 copies it with one thread byte by byte; how long
    that takes is not measured, so it is not tested here.)"""
    set_mode(monkeypatch, checked)
    big = b"m" * 7 + bytes(range(1, 256)) * ((1 << 24) // 255) + b"q" * 64
    big = big[: 1 << 24]
    words = [b"z", big, b"mmmmmmm", b"a", b"mmmmmmm\x01\x02\x03"]
    e = engine()
    try:
        assert_sorts(e, words, [5, 4, 3, 2, 1])
        assert b"a word of 16 MiB or more" in e._L.mox_last_error()
    finally:
        e.close()


CHILD = r"""
import sys
sys.path[:0] = [%r, %r, %r]
import numpy as np, bsort_cases as C, coracle, mox
from mox import corpus
from test_gpu_bsort import assert_sorts
""" % (os.path.join(ROOT, "map-oxidize_amd"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests"))


def run_child(body, checked, **env):
    env = dict(os.environ, MOX_VERBOSE="1", **env)
    env.pop("MOX_BSORT_CHECKED", None)
    if checked:
        env["MOX_BSORT_CHECKED"] = "1"
    r = subprocess.run([sys.executable, "-c", CHILD + body], env=env, capture_output=True, timeout=240, cwd=ROOT)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    assert b"child ok" in r.stdout
    return bsort_lines(r.stderr.decode())


@MODES
def test_one_region_forced(checked):
    """MOX_BSORT_ONE_REGION=1: one look-back status region, zeroed again before
    every digit pass, as tables past 256 MiB of status words use it (else only
    the 16 GiB slow test does): two tiles + 1, and the checked radix on 10 digits."""
    lines = run_child(r"""
e = mox.Engine(device=0, flags=mox.MOX_F_SORT_BYTES)
assert_sorts(e, C.run_geometry_over())
assert_sorts(e, C.sizes(2 * C.OS_TILE + 1))
e.close()
print("child ok")
""", checked, MOX_BSORT_ONE_REGION="1")
    assert [ln["checked"] for ln in lines] == ([1, 1] if checked else [0, 1, 0])
    assert all(ln["one_region"] == 1 for ln in lines)


@MODES
def test_borrowed_pass_buffers(checked):
    """MOX_BSORT_TMP_MAX: the first scratch request counts as failed, so the
    record arrays borrow the pass buffers that are dead once the table is built
    (else only the 16 GiB slow test does).  The sorted table equals the oracle's
    array for array; the same engine then counts another corpus exactly: the
    pass gets its buffers back and rebuilds what the sort overwrote."""
    lines = run_child(r"""
e = mox.Engine(device=0, flags=mox.MOX_F_SORT_BYTES, reserve_bytes=24 << 20)
first = corpus.fill(corpus.HICARD, 95, 0, 24 << 20)
z = corpus.fill(corpus.ZIPF, 96, 0, 8 << 20)
h = corpus.fill(corpus.HICARD, 97, 0, 12 << 20)
second = np.concatenate([z, np.frombuffer(b" \n", np.uint8), h])
for data in (first, second):
    t = e.count(data.tobytes())
    counts, offs, raw = t.arrays()
    t.close()
    wc, wo, wraw, _ = coracle.count_arrays(data, nthreads=16)
    assert np.array_equal(counts, wc) and np.array_equal(offs, wo) and raw == wraw
e.close()
print("child ok")
""", checked, MOX_BSORT_TMP_MAX=str(1 << 20))
    assert len(lines) >= 2 and (not checked or all(ln["checked"] == 1 for ln in lines))
    for ln in lines:  # both sorts borrow; A, B, pay, fin, pos (and S when checked) are the big arrays
        k, m = ln["borrowed"]
        assert k >= 1 and m == (6 if checked else 5), lines
    assert lines[0]["n"] > C.OS_TILE  # more than one tile: the look-back runs in borrowed buffers
