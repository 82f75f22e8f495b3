"""GPU: the reduce half of the pass (k_split_count, k_split_scatter, k_reduce,
k_reduce_small, k_reduce_sort1 / 2 in map-oxidize_amd/csrc/mox_kernels.hip) on
the corpora of reduce_cases.py, each built from words with chosen key hashes
to land exactly on one of the path's unit cut-offs (the CPU tests in
test_reduce_model.py assert that geometry).  Every corpus is under 1 MiB.

Every test asserts
  exactness: the fetched table equals the C oracle's, word for word and count
      for count;
  order: the table in engine order lists its words in the model's key_less
      order (h32, hash32b, w0, w1) -- any wrong bit of the restated hash32 or
      hash32b reorders it, and the order does not depend on which kernel
      reduced a unit;
  geometry: the last `attempt` line the engine prints under MOX_VERBOSE (units,
      sort2 / k_reduce / k_reduce_small lists, split partitions, sub-passes)
      and mox_stats' cold and weighted records equal the model's prediction,
      with nothing spilled -- the cut-off was reached, not just approached.

Case -> what it reaches <- the CPU assertion that guarantees it:
  unit_sizes -> the list rule of k_split_scatter at 0, 1, 64, 65, 511, 512 | 513, 1023, 1024 | 1025
      cold records; one-word units of 512 and 1024; repeats across a lane <- test_unit_sizes_details
  sort_key_ties -> sort_reduce_unit's 64-bit re-sort (keys sharing all 23 / 22 sort-key bits) and
      equal h32 told apart by hash32b in the first sort <- test_sort_key_ties_details
  weighted_mix -> 511 + 1 (k_reduce_small at SMALL_CAP), 512 + 1 (k_reduce), weighted-only units of
      40, 512 and 513 records, a whole partition of weighted records only <- test_case_geometry
  split_min_edge[_over] -> SPLIT_MIN records stay whole in 4 sub-passes of RED_CAP keys (over:
      RED_CAP + 1 in one: 8), SPLIT_MIN + 1 split <- test_case_geometry
  red_cap_edge[_over] -> RED_CAP keys in one pass, RED_CAP + 1 in two, once and three times each
  bucket_clusters -> red_insert's walk: 9, 12, 40 keys under one tag, 40 in one bucket, bucket
      RED_BK - 1 -> spare -> 0, 100 keys in one sort bin <- test_bucket_clusters_details
  small_table_clusters -> k_reduce_small: a 100-key chain, a chain wrapping at SR_TSLOTS - 1, one
      word as 300 weighted records <- test_small_table_clusters_details
  hash_zero, dictionary_same_hash -> raw hashes 0 and 1 and four hot words on two dictionary
      slots, rare and hot (exactness, order, dict_words) <- test_hash_zero_and_dictionary_details
  pairs_split_min -> mox_reduce_pairs: SPLIT_MIN whole, SPLIT_MIN + 1 split, weighted units of 512
      and 513, duplicate words, 64-bit counts <- test_pairs_case_details

Every corpus case runs on a default engine and on a MOX_F_NO_DICT engine.  A
case whose repeated words would fill a dictionary says what the default engine
may assert (Case.default_engine): "lists" (the partitions stay whole whatever
the dictionary takes), "hot" (unit_sizes: the dictionary takes exactly its two
one-word units' words, which leaves the partition whole with 16 sub-passes --
the round-6 regime of whole partitions of 2,049 .. 8,192 distinct records) or
"exact" (exactness, order and dict_words only; without
a dictionary the hot words of these two cases overflow a region slice and
spill, which is correct and changes the record kinds).

Not covered: full (h32, hash32b) collisions (the forced-collision build,
test_gpu_collide.py); kk other than 5 and partitions near a kk boundary (kk
follows a sampled estimate through __logf); units of more than RED_CAP keys
inside a split partition; k_xsplit at more than 16 ranks; a map grid other than
256 workgroups (region_fill models that grid: on another device a spill would
fail the geometry assertions, not exactness).  The long-word table, the spill
path under overflow and the buffer-growth retries: test_gpu_growth.py."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import coracle
import mox
import reduce_cases as R
from conftest import ROOT, assert_tables_equal

pytestmark = pytest.mark.gpu

LINE = re.compile(r"^\[mox\] (reduce-only )?attempt (\d+): overflow 0x([0-9a-f]+) (?:cold_need \d+ spill_need (\d+) )?.*?"
                  r"units (\d+), sort2 list (\d+), k_reduce list (\d+), k_reduce_small list (\d+), "
                  r"split partitions (\d+), max sub-passes (\d+)$", re.M)


# the counters and capacities of a map + reduce pass's line (test_gpu_growth.py)
CAPS = re.compile(r"cold_need (\d+) spill_need \d+ w_total (\d+) u_n (\d+) n_total (\d+) caps cold (\d+) spill (\d+) w (\d+)"
                  r"(?: u (\d+) arena (\d+) long (\d+) table (\d+) bytes (\d+))? run ")
CAPS_KEYS = ("cold_need", "w_total", "u_n", "n_total", "cold", "spill", "w", "u", "arena", "long", "table", "bytes")


def attempt_lines(err, reduce_only=False):
    """The engine's MOX_VERBOSE lines of the map + reduce pass (or of the
    reduce-only pass) as dicts, in the order printed."""
    out = []
    for m in LINE.finditer(err):
        if bool(m.group(1)) != reduce_only:
            continue
        c = CAPS.search(m.group(0))
        out.append({"attempt": int(m.group(2)), "overflow": int(m.group(3), 16), "spill_need": int(m.group(4) or 0),
                    "units": int(m.group(5)), "sort2": int(m.group(6)), "k_reduce": int(m.group(7)),
                    "k_reduce_small": int(m.group(8)), "split": int(m.group(9)), "max_sub": max(1, int(m.group(10)))})
        if c:
            out[-1].update({k: int(v) for k, v in zip(CAPS_KEYS, c.groups()) if v is not None})
    return out


LISTS = ("units", "sort2", "k_reduce", "k_reduce_small", "split", "max_sub")


def assert_geometry(line, case, want=None):
    want = want or case.geometry.summary()
    print("%s: line %r, model %r" % (case.name, line, want))
    assert line["overflow"] == 0 and line["spill_need"] == 0
    assert {k: line[k] for k in LISTS} == {k: want[k] for k in LISTS}


def assert_exact_and_ordered(table, text, case):
    """table: Table.arrays() and Table.items() of the fetched result."""
    arrays, items = table
    wc, wo, wraw, _ = coracle.count_arrays(np.frombuffer(text, np.uint8), nthreads=16)
    assert_tables_equal(arrays, (wc, wo, wraw))
    assert dict(items) == case.expected()
    got, want = [w for w, _ in items], R.model_order(case.words())
    if got != want:
        j = next(i for i, (a, b) in enumerate(zip(got, want)) if a != b)
        raise AssertionError("table order leaves the model's at %d of %d: %r (key %r), want %r (key %r)" % (
            j, len(want), got[j], R.order_key(got[j]), want[j], R.order_key(want[j])))


def count(text, flags=0, lib_path=None):
    """(arrays, items), stats and the attempt lines of one fresh engine's pass."""
    e = mox.Engine(device=0, flags=flags, reserve_bytes=R.RESERVE, lib_path=lib_path)
    try:
        t = e.count(text)
        try:
            table = (t.arrays(), list(t.items()))
            tokens = t.tokens
        finally:
            t.close()
        st = e.stats()
    finally:
        e.close()
    assert tokens == st["tokens"]
    return table, st


@pytest.mark.parametrize("dictionary", [True, False], ids=["dict", "nodict"])
@pytest.mark.parametrize("name", list(R.CORPUS_CASES))
def test_corpus_case(monkeypatch, capfd, name, dictionary):
    case = R.case(name)
    text = case.text()
    monkeypatch.setenv("MOX_VERBOSE", "1")
    capfd.readouterr()
    table, st = count(text, 0 if dictionary else mox.MOX_F_NO_DICT)
    lines = attempt_lines(capfd.readouterr().err)
    assert_exact_and_ordered(table, text, case)
    want = case.geometry.summary()
    assert st["tokens"] == want["cold_records"] + want["weighted_records"]
    print("%s: stats %r" % (name, {k: st[k] for k in ("dict_words", "cold_records", "weighted_records", "retries",
                                                      "reduce_units", "split_partitions", "max_subpasses")}))
    assert lines and lines[-1]["attempt"] == st["retries"]
    mode = case.default_engine if dictionary else ("same" if case.default_engine != "exact" else "exact")
    if mode == "exact":
        if dictionary:  # the hot words are in the dictionary (it may also admit rare ones)
            assert st["dict_words"] >= R.dict_placed(case.hot)
        else:
            assert st["dict_words"] == 0
        return
    if mode == "hot":  # the dictionary takes the hot words and no other: one weighted record each
        want = case.dict_geometry.summary()
    assert_geometry(lines[-1], case, want)
    assert (st["reduce_units"], st["split_partitions"], st["max_subpasses"]) == (want["units"], want["split"], want["max_sub"])
    if mode in ("same", "hot"):
        assert st["dict_words"] == (len(case.hot) if mode == "hot" else 0)
        assert (st["cold_records"], st["weighted_records"]) == (want["cold_records"], want["weighted_records"])


@pytest.mark.parametrize("name", list(R.PAIRS_CASES))
def test_pairs_case(monkeypatch, capfd, name):
    """mox_reduce_pairs: every record weighted, the reduce-only pass."""
    case = R.case(name)
    monkeypatch.setenv("MOX_VERBOSE", "1")
    e = mox.Engine(device=0)
    try:
        capfd.readouterr()
        t = e.reduce_pairs([w for w, _ in case.pairs], [n for _, n in case.pairs])
        try:
            items = list(t.items())
        finally:
            t.close()
        lines = attempt_lines(capfd.readouterr().err, reduce_only=True)
        st = e.stats()
    finally:
        e.close()
    assert dict(items) == case.expected() and len(items) == len(case.expected())
    assert [w for w, _ in items] == R.model_order(case.words())
    assert st["weighted_records"] == len(case.pairs)
    assert lines
    assert_geometry(lines[-1], case)


def test_unit_sizes_through_the_exchange(monkeypatch, capfd):
    """Two ranks, each owning one copy of unit_sizes: both local passes split
    the partition into the case's units (k_xpack_short then packs index-form
    units of 1, 512, 513 and 1024 records), and the reduce-only pass over what
    was packed sums the two copies."""
    import test_gpu_exchange as X
    case = R.case("unit_sizes")
    text = case.text()
    assert text[-1:].isspace()
    data = text + text
    monkeypatch.setenv("MOX_VERBOSE", "1")
    capfd.readouterr()
    stats = []
    out = X.run_ranks(data, 2, stats=stats, table_order=True, flags=mox.MOX_F_NO_DICT, reserve_bytes=R.RESERVE)
    err = capfd.readouterr().err
    local, final = attempt_lines(err), attempt_lines(err, reduce_only=True)
    done = [ln for ln in local if ln["overflow"] == 0]
    assert len(done) == 2
    for ln in done:
        assert_geometry(ln, case)
    print("reduce-only lines: %r" % (final,))
    assert len([ln for ln in final if ln["overflow"] == 0]) == 2
    items = [kv for part, _ in out for kv in part]
    assert sorted(items) == coracle.count(data, nthreads=16)[0]
    assert dict(items) == {w: 2 * n for w, n in case.expected().items()}
    for part, _ in out:  # every rank's table in the order of the reduce kernels
        assert [w for w, _ in part] == R.model_order([w for w, _ in part])
    assert sum(tok for _, tok in out) == 2 * sum(n for _, n, _ in case.items)


def test_check_build_runs_the_edges_clean():
    """unit_sizes, weighted_mix and bucket_clusters under the bounds-check build
    (libmox_check.so: every derived index of the split / reduce kernels checked
    on the device, the k_reduce table invariants after every unit): clean and
    exact, with and without a dictionary."""
    code = r"""
import sys
sys.path[:0] = [%r, %r, %r]
import mox, reduce_cases as R
import test_gpu_reduce_edges as T
for name in ("unit_sizes", "weighted_mix", "bucket_clusters"):
    case = R.case(name)
    text = case.text()
    for flags in (0, mox.MOX_F_NO_DICT):
        table, st = T.count(text, flags)
        T.assert_exact_and_ordered(table, text, case)
print("check build clean")
""" % (os.path.join(ROOT, "map-oxidize_amd"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests"))
    env = dict(os.environ, MOX_LIB=mox.CHECK_LIB_PATH)
    env.pop("MOX_VERBOSE", None)
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, timeout=240, cwd=ROOT)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    assert b"check build clean" in r.stdout
