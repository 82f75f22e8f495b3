"""GPU: the buffer-growth ladder of run_corpus (mox_engine.hip: initial_caps,
grow_for, cold_cap_for, GROW_RETRIES), the map's spill path (cold_spill ->
k_hist / k_scatter -> weighted records) and the long-word table (long_insert,
ref_byte) on the corpora of growth_cases.py.  Every case is one fresh engine
with no reserve, so the pass starts from initial_caps of its text (at most
2 MiB) and has to find every capacity it is short of through Ctl::overflow.
test_growth_model.py asserts on the CPU that each case is short of what it
names; here the engine's MOX_VERBOSE attempt lines are compared with the
ladder the host model predicts.

Every case asserts
  exactness: the fetched table equals the C oracle's, and so do the tokens;
  ladder: attempt by attempt, the overflow mask, the capacities (cold, spill, w,
      u, arena, long, table, bytes) and the counters cold_need, spill_need,
      w_total and u_n on the line equal the model's; stats.retries is the
      number of lines - 1; the last line's n_total and mox_stats' records are
      the model's.  A wrong coefficient in the restated grow_for moves a
      capacity, a wrong overflow rule a mask.

Case -> what it reaches (ladder) <- the CPU assertion that guarantees it:
  table_alone, bytes_alone, u_alone, arena_alone, w_alone -> one bit alone, cured in one
      step <- test_alone_case_exceeds_its_capacity_and_no_other
  long_fill -> a full long table probed end to end by 64 more words (OVF_LONG), regrown to
      another mask, then OVF_BYTES <- test_long_fill_details
  arena_alone -> tokens of the letters that grow from 2 to 3 bytes fill their reservation of
      len + len / 2 + 4 to 4 bytes <- test_arena_alone_reservation_is_exactly_tight
  pool_ladder -> OVF_POOL | OVF_W, OVF_W, 0; a second count on the same engine starts at the
      learnt capacities: no overflow, no retry <- test_pool_ladder_second_run_...; w_alone's
      second count shows next_cold_cap on its own (regions of 64 grow to 72 with no overflow)
  spill_edges_nodict / _dict -> region fills of rc - 1, rc, rc + 1, rc + 2 (cold_pair's pair at
      the edge, the parked single at pos == rc, a pair that spills whole; with a dictionary
      the single-record path at rc = 64): 3 spills, no overflow <- test_spill_edges_details
  long_refs -> one long word by corpus and by arena reference (KELVIN SIGN lowers to k), words
      that differ in the last byte, a NUL byte, 16 | 17 bytes <- test_long_refs_oracle
  ladder_all -> short of everything at once: converges inside GROW_RETRIES, every line but the
      last overflows, the union of the masks is the model's; the sequence itself is printed,
      not asserted (the second OVF_SPLIT stage follows a sampled estimate)

mox_stats.weighted_records is Ctl::w_n, the records the dictionary and the
Unicode lane asked for; the spills join them in w_total (the attempt line).
spill_edges_dict therefore asserts weighted_records = dict_words + Unicode
tokens and w_total = dict_words + Unicode tokens + spills.

Out of scope: OVF_PROBE (2^24 spins on one slot); OVF_REDUCE (the
forced-collision build's ground, test_gpu_collide.py); the uniq_cap arm of
OVF_POOL (out of reach at these sizes: test_ladder_converges_as_claimed); the
growth of the async path and of the overlapped file path (test_gpu_parity.py)
and of the reduce-only pass, which sizes its buffers from the received counts.
A map grid other than 256 workgroups: the model is of that grid, on another
device the ladder assertions fail, not exactness."""
import os
import subprocess
import sys

import numpy as np
import pytest

import coracle
import growth_cases as G
import mox
from conftest import ROOT, assert_tables_equal
from growth_cases import C
from test_gpu_reduce_edges import attempt_lines

pytestmark = pytest.mark.gpu

LADDER_CASES = [n for n in G.CASES if n != "ladder_all"]
DICT_FREE = ("table_alone", "bytes_alone", "long_fill", "u_alone", "arena_alone")
TWICE = {"pool_ladder": 80, "w_alone": 72}  # counted twice on one engine: the second count's region capacity
LINE_KEYS = ("overflow", "cold", "spill", "w", "u", "arena", "long", "table", "bytes", "cold_need", "spill_need", "w_total", "u_n")


def run_case(case, runs=1, lib_path=None):
    """`runs` counts of the case's text on one fresh engine: [(table, stats)],
    table = (arrays, items, tokens)."""
    e = mox.Engine(device=0, flags=mox.MOX_F_NO_DICT if case.nodict else 0, reserve_bytes=0, lib_path=lib_path)
    out = []
    try:
        for _ in range(runs):
            t = e.count(case.text)
            try:
                table = (t.arrays(), list(t.items()), t.tokens)
            finally:
                t.close()
            out.append((table, e.stats()))
    finally:
        e.close()
    return out


def assert_exact(table, case):
    arrays, items, tokens = table
    if b"\0" in case.text:  # (assert_tables_equal's fixed-width words hold no NUL byte)
        want, wtok = coracle.count(case.text, nthreads=16)
        assert sorted(items) == want
    else:
        wc, wo, wraw, wtok = coracle.count_arrays(np.frombuffer(case.text, np.uint8), nthreads=16)
        assert_tables_equal(arrays, (wc, wo, wraw))
    assert tokens == wtok == case.figures.tokens


def model_line(h, caps):
    return dict({k: caps[k] for k in ("cold", "spill", "w", "u", "arena", "long", "table", "bytes")},
                **{k: h[k] for k in ("overflow", "cold_need", "spill_need", "w_total", "u_n")})


def show(name, lines, ladder=None):
    for i, ln in enumerate(lines):
        print("%s attempt %d: %s %r" % (name, i, G.mask_names(ln["overflow"]), {k: ln.get(k) for k in LINE_KEYS + ("n_total",)}))
        if ladder is not None and i < len(ladder):
            print("%s   model %d: %s %r" % (name, i, G.mask_names(ladder[i][0]["overflow"]), model_line(*ladder[i])))


def assert_ladder(name, lines, ladder, st):
    show(name, lines, ladder)
    assert [ln["attempt"] for ln in lines] == list(range(len(lines)))
    assert [ln["overflow"] for ln in lines] == [h["overflow"] for h, _ in ladder]
    for ln, (h, caps) in zip(lines, ladder):
        assert {k: ln[k] for k in LINE_KEYS} == model_line(h, caps)
    assert st["retries"] == len(lines) - 1
    h = ladder[-1][0]
    assert lines[-1]["n_total"] == h["n_total"] == st["uniques"]
    print("%s: stats %r" % (name, {k: st[k] for k in ("tokens", "uniques", "dict_words", "cold_records", "weighted_records",
                                                      "unicode_tokens", "long_tokens", "chunks", "retries")}))
    assert (st["unicode_tokens"], st["long_tokens"], st["chunks"]) == (h["u_n"], h["long_n"], h["cold_need"])


@pytest.mark.parametrize("name", LADDER_CASES)
def test_growth_ladder(monkeypatch, capfd, name):
    case = G.case(name)
    model = G.EngineModel()
    ladder = model.run(case.figures)
    monkeypatch.setenv("MOX_VERBOSE", "1")
    capfd.readouterr()
    runs = run_case(case, runs=2 if name in TWICE else 1)
    lines = attempt_lines(capfd.readouterr().err)
    (table, st) = runs[0]
    first = lines[:st["retries"] + 1]
    assert_exact(table, case)
    assert_ladder(name, first, ladder, st)
    h = ladder[-1][0]
    if name in DICT_FREE or case.nodict:
        assert st["dict_words"] == 0
    if name.startswith("spill_edges"):
        cl = case.claims
        assert st["dict_words"] == len(case.dictionary)
        assert (st["cold_records"], st["weighted_records"]) == (h["cold_recs"], h["w_n"])
        assert st["weighted_records"] == st["dict_words"] + cl["unicode"]
        assert first[-1]["w_total"] == st["dict_words"] + cl["unicode"] + cl["spills"]
        assert first[-1]["spill_need"] == 2 and first[-1]["overflow"] == 0
    elif name != "long_refs":  # (long_refs' few short words form a dictionary on a text this small)
        assert (st["cold_records"], st["weighted_records"]) == (h["cold_recs"], h["w_n"])
    if name in TWICE:
        # the second count of the same text: the capacities the first ended with, the
        # region capacity what cold_cap_for learnt from its spills (w_alone: the first
        # count never met OVF_POOL, so only next_cold_cap moves its regions, 64 -> 72)
        learnt = model.next_cold_cap
        again = model.run(case.figures)
        (table2, st2), second = runs[1], lines[len(first):]
        assert len(again) == 1
        assert_exact(table2, case)
        assert_ladder(name + " (second count)", second, again, st2)
        assert len(second) == 1 and second[0]["overflow"] == 0 and st2["retries"] == 0
        assert second[0]["cold"] == G.realloc_sized(dict(again[0][1], cold=learnt))["cold"] == TWICE[name]
    else:
        assert len(lines) == len(first)


def test_ladder_all_converges(monkeypatch, capfd):
    case = G.case("ladder_all")
    ladder = G.ladder_of(case)
    monkeypatch.setenv("MOX_VERBOSE", "1")
    capfd.readouterr()
    (table, st), = run_case(case)
    lines = attempt_lines(capfd.readouterr().err)
    show("ladder_all", lines, ladder)
    print("ladder_all: %d retries (GROW_RETRIES %d): %s; model %s" % (
        st["retries"], C.GROW_RETRIES, [G.mask_names(ln["overflow"]) for ln in lines], [G.mask_names(h["overflow"]) for h, _ in ladder]))
    assert_exact(table, case)
    assert st["retries"] == len(lines) - 1 <= C.GROW_RETRIES
    assert all(ln["overflow"] for ln in lines[:-1]) and lines[-1]["overflow"] == 0
    union = 0
    for ln in lines:
        union |= ln["overflow"]
    assert union == case.claims["union"]
    assert lines[-1]["n_total"] == case.figures.n_total == st["uniques"]
    assert st["split_partitions"] >= 1 and st["dict_words"] == 0


CHECK_CASES = ("spill_edges_nodict", "spill_edges_dict", "pool_ladder", "long_fill", "long_refs")


def test_check_build_runs_the_growth_cases_clean():
    """The spill and long-table cases under the bounds-check build
    (libmox_check.so: CHK_SCATTER guards k_scatter's writes of the spills, the
    table kernels check every derived offset): no MOX_EHIP, exact tables."""
    if not os.path.exists(mox.CHECK_LIB_PATH):
        pytest.skip("libmox_check.so is not built (make check)")
    code = r"""
import sys
sys.path[:0] = [%r, %r, %r]
import growth_cases as G
import test_gpu_growth as T
for name in %r:
    case = G.case(name)
    (table, st), = T.run_case(case)
    T.assert_exact(table, case)
    print(name, "retries", st["retries"])
print("check build clean")
""" % (os.path.join(ROOT, "map-oxidize_amd"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests"), CHECK_CASES)
    env = dict(os.environ, MOX_LIB=mox.CHECK_LIB_PATH)
    env.pop("MOX_VERBOSE", None)
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, timeout=240, cwd=ROOT)
    print(r.stdout.decode())
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    assert b"check build clean" in r.stdout
