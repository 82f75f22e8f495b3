"""CPU: the capacity and attempt model of growth_cases.py and the cases
test_gpu_growth.py runs, so that a GPU test there cannot pass without meeting
the overflow it is there for.  The constants are parsed from the sources; every
*_alone case is checked to exceed the capacity it names and no other (every
figure is printed next to its capacity), every ladder to end inside
GROW_RETRIES, spill_edges to land on the fills it names, and the C oracle to
count every corpus to the table the model plans.  No GPU code runs here."""
import numpy as np
import pytest

import coracle
import growth_cases as G
import pyoracle
import reduce_cases as R
from growth_cases import C
from reduce_cases import K

ALL = list(G.CASES)
DICT_FREE = ("table_alone", "bytes_alone", "long_fill", "u_alone", "arena_alone")  # default engine, no dictionary forms


def test_parsed_constants():
    """The cases are laid out for these values: a change in the sources fails
    here first."""
    got = {n: getattr(C, n) for n in ("NB", "QF_MAX", "COLD_CAP_MAX", "SPLIT_PER_REGION", "SUB_N", "SPLIT_MIN", "GROW_RETRIES",
                                      "PAY")}
    assert got == {"NB": 1024, "QF_MAX": 4, "COLD_CAP_MAX": 262144, "SPLIT_PER_REGION": 4, "SUB_N": 4096, "SPLIT_MIN": 8192,
                   "GROW_RETRIES": 8, "PAY": 992}
    assert C.OVF == {"POOL": G.OVF_POOL, "W": G.OVF_W, "U": G.OVF_U, "LONG": G.OVF_LONG, "ARENA": G.OVF_ARENA,
                     "PROBE": G.OVF_PROBE, "TABLE": G.OVF_TABLE, "BYTES": G.OVF_BYTES, "REDUCE": G.OVF_REDUCE,
                     "SPLIT": G.OVF_SPLIT}
    assert C.COLD_CAP_MAX % (2 * C.QF_MAX) == 0 and G.GRID * C.QF_MAX <= K.MAX_MAP_GRID  # hc_qf: four slices


def test_restated_formulas_still_read_as_the_sources_do():
    """The coefficients restated in growth_cases.py, found in the host and
    kernel code they restate."""
    eng, ker = R._source("mox_engine.hip"), K._k
    for text in ("std::max<uint64_t>(64, n / ((uint64_t)map_grid * NB * 8))", "std::max<uint64_t>(1024, n / ((uint64_t)map_grid * 64))",
                 "c.w_cap = 65536 + n / 64;", "c.u_cap = 4096 + n / 64;", "c.arena_cap = 65536 + n / 16;", "c.long_cap = 65536;",
                 "c.table_cap = 65536 + n / 64;", "c.bytes_cap = c.table_cap * 8;",
                 "h.cold_need + h.cold_need / 8 + 16", "4 * h.tokens / ((uint64_t)e->w.map_grid * NB) + 64",
                 "h.spill_need + h.spill_need / 4 + 1024", "wn + wn / 4 + 1024", "h.u_n + h.u_n / 4 + 1024",
                 "h.arena_n + h.arena_n / 4 + 65536", "next_pow2(2 * h.long_n + 1024)", "h.n_total + h.n_total / 4 + 1024",
                 "h.bytes_total + h.bytes_total / 4 + 65536", "h.split_k + h.split_k / 8 + 4096",
                 "h.cold_recs + h.cold_recs / 8 + (uint64_t)NB * (SUB_N + 2)", "need.table_cap * 16",
                 "(c.cold_cap + 2 * QF_MAX - 1) & ~(uint64_t)(2 * QF_MAX - 1)", "n.long_cap = next_pow2(c.long_cap);",
                 "n.uniq_cap = (uint64_t)n.map_grid * NB * n.cold_cap + c.w_cap;", "if (attempt >= GROW_RETRIES)",
                 "if (h.spill_need) e->next_cold_cap"):
        assert text in eng, text
    for text in ("uint64_t cap = r.len + r.len / 2 + 4;", "if (ao + cap > w.arena_cap)", "if (pos + 1 < m.rc)",
                 "atomicAdd(&m.s.bcnt[B], 2u)", "cnt < m.rc ? cnt : m.rc", "sn < w.spill_cap ? sn : w.spill_cap",
                 "if (++probes > mask)", "if (sw > w.w_cap)", "if (ns + nl > w.table_cap)", "if (sb + lb > w.bytes_cap)",
                 "if (tk > w.split_k_cap || tw > w.split_w_cap)", "(n + (1ull << kk) + 1) & ~1ull"):
        assert text in ker, text


def test_capacity_model_known_values():
    """The table of the initial capacities at n = 1 MiB on 256 workgroups, and
    the roundings of realloc_sized."""
    c = G.initial_caps(1 << 20)
    assert c == {"cold": 64, "spill": 1024, "w": 65536 + 16384, "u": 4096 + 16384, "arena": 65536 + 65536, "long": 65536,
                 "table": 65536 + 16384, "bytes": 8 * (65536 + 16384), "split_k": 0, "split_w": 0}
    assert G.initial_caps(256 << 20)["cold"] == R.COLD_CAP
    r = G.realloc_sized(dict(c, cold=67, long=65537))
    assert (r["cold"], r["long"]) == (72, 131072)
    assert G.realloc_sized(dict(c, cold=1 << 20))["cold"] == C.COLD_CAP_MAX
    have, re_ = G.ensure_caps(r, dict(c, cold=70))
    assert have is r and not re_
    have, re_ = G.ensure_caps(r, dict(c, table=c["table"] + 1))
    assert re_ and have["table"] == c["table"] + 1 and have["cold"] == 72 and have["long"] == 131072
    h = {"cold_need": 17856, "tokens": 1 << 20, "overflow": 0}
    assert G.cold_cap_for(dict(c), h) == 80 and G.cold_cap_for(dict(c, cold=4096), h) == 4096
    assert G.cold_cap_for(dict(c), dict(h, cold_need=40)) == 61


def needs_against_caps(fig, caps):
    """{buffer: (what the text needs, its capacity)} for the buffers with an
    overflow bit of their own."""
    spills = fig.spills_per_wg(caps["cold"])
    return {"spill": (int(spills.max()), caps["spill"]), "w": (fig.dict_hit_words + fig.u_short_n + int(spills.sum()), caps["w"]),
            "u": (fig.u_n, caps["u"]), "arena": (fig.u_arena, caps["arena"]), "long": (len(fig.long_words), caps["long"]),
            "table": (fig.n_total, caps["table"]), "bytes": (fig.bytes_total, caps["bytes"])}


@pytest.mark.parametrize("name", G.ALONE)
def test_alone_case_exceeds_its_capacity_and_no_other(name):
    case = G.case(name)
    fig = case.figures
    needs = needs_against_caps(fig, G.realloc_sized(G.initial_caps(fig.n)))
    for k, (need, cap) in needs.items():
        print("%s: %-6s needs %9d of %9d%s" % (name, k, need, cap, "  <- over" if need > cap else ""))
    assert {k for k, (need, cap) in needs.items() if need > cap} == {case.targets}
    assert len(case.text) <= 2 << 20


@pytest.mark.parametrize("name", ALL)
def test_ladder_converges_as_claimed(name):
    case = G.case(name)
    ladder = G.ladder_of(case)
    print("%s (%d bytes): %s" % (name, len(case.text), G.describe(ladder)))
    masks = [h["overflow"] for h, _ in ladder]
    assert masks[-1] == 0 and all(masks[:-1]) and len(ladder) - 1 <= C.GROW_RETRIES
    if case.claimed is not None:
        assert masks == case.claimed
    assert len(case.text) <= 2 << 20
    for h, caps in ladder:  # the uniq_cap arm of OVF_POOL is out of reach at these sizes
        assert h["cold_recs"] + h["w_total"] <= G.uniq_cap(caps)


@pytest.mark.parametrize("name", ALL)
def test_oracle_counts_the_planned_table(name):
    """Tokens, distinct words and table bytes of the model are the C oracle's."""
    case = G.case(name)
    counts, offs, raw, tokens = coracle.count_arrays(np.frombuffer(case.text, np.uint8), nthreads=16)
    fig = case.figures
    assert (tokens, counts.size, int(offs[-1])) == (fig.tokens, fig.n_total, fig.bytes_total)
    assert int(counts.sum()) == fig.tokens


@pytest.mark.parametrize("name", ["u_alone", "arena_alone", "long_refs", "spill_edges_dict"])
def test_model_lowers_as_the_oracle_does(name):
    fig = G.case(name).figures
    n = 0
    for tok, low in zip(fig.distinct_tokens, fig.low):
        if max(tok) >= 0x80:
            assert coracle.lowercase(tok) == low
            n += 1
    assert n


@pytest.mark.parametrize("name", DICT_FREE)
def test_no_dictionary_forms_on_a_default_engine(name):
    """No short ASCII word is sampled twice (the pieces do not overlap), so
    k_dict_pick takes nothing."""
    case = G.case(name)
    assert not case.nodict
    picked, _ = G.dictionary_pick(case.text)
    assert picked == []
    counts = G.sample_counts(case.text)
    assert max(counts.values(), default=0) <= 1


def test_arena_alone_reservation_is_exactly_tight():
    case = G.case("arena_alone")
    fig = case.figures
    grown = 0
    for tok, low in zip(fig.distinct_tokens, fig.low):
        assert len(tok) == 2 * G.ARENA_CHARS and len(low) <= len(tok) + len(tok) // 2 + 4
        if len(low) == len(tok) + len(tok) // 2:
            grown += 1
            assert set(tok.decode("utf-8")) <= set(G.GROWING)
        else:
            assert len(low) == len(tok)
    assert grown == case.claims["growing"] == len(fig.distinct_tokens) // 3
    assert fig.u_n == G.ARENA_TOKENS and len(fig.long_words) == len(fig.distinct_tokens) == 72 and fig.u_short_n == 0


def test_long_fill_details():
    case = G.case("long_fill")
    fig = case.figures
    assert len(fig.long_words) == case.claims["distinct"] == 65536 + G.LONG_EXTRA
    assert fig.ascii_long_n == case.claims["long_tokens"] == 65536 + 2 * G.LONG_EXTRA
    assert all(len(w) == 17 for w in fig.long_words)
    assert sum(1 for t in fig.distinct_tokens if t != t.lower()) == G.LONG_EXTRA
    (h0, c0), (h1, c1), _ = G.ladder_of(case)
    assert c0["long"] == 65536 < len(fig.long_words) and c1["long"] == 1 << 18  # full, then another mask


@pytest.mark.parametrize("dictionary", [False, True], ids=["nodict", "dict"])
def test_spill_edges_details(dictionary):
    case = G.case("spill_edges_dict" if dictionary else "spill_edges_nodict")
    fig, cl = case.figures, case.claims
    rc = cl["rc"]
    caps = G.realloc_sized(G.initial_caps(fig.n))
    assert caps["cold"] // fig.qf == rc and fig.qf == (1 if dictionary else C.QF_MAX)
    fills = fig.fills()
    want = {(g, cl["part"], cl["slice"]): f for g, f in cl["fills"].items()}
    assert sorted(want.values()) == [rc - 1, rc, rc + 1, rc + 2] and len({g for g, _, _ in want}) == 4
    for k, f in want.items():
        assert fills[k] == f
    others = [f for k, f in fills.items() if k not in want]
    print("%s: rc %d, planted %r, largest other fill %d" % (case.name, rc, want, max(others, default=0)))
    assert max(others, default=0) < rc - 1
    h = fig.attempt(caps)
    assert (h["overflow"], h["spills"], h["spill_need"]) == (0, cl["spills"], 2)
    assert fig.u_n == cl["unicode"] == fig.u_short_n
    # every planted word is there once, in the first row of its workgroup
    assert h["cold_recs"] + h["spills"] == (sum(want.values()) if dictionary else fig.tokens)
    if not dictionary:
        assert case.nodict and h["w_total"] == 3 and h["w_n"] == 0
        return
    # the dictionary gate: the hot words repeat, nothing else does
    hot = case.dictionary
    picked, (cov, cov_all) = G.dictionary_pick(case.text)
    counts = G.sample_counts(case.text)
    repeat = sum(c for c in counts.values() if c > 1) / float(sum(counts.values()))
    print("spill_edges_dict: %d hot words, sampled repeat fraction %.3f, gate %d of %d" % (len(hot), repeat, cov, cov_all))
    assert sorted(picked) == sorted(hot) and len(hot) == 40
    assert repeat > 1.0 / K.DICT_MIN_COVER_INV and cov >= cov_all // K.DICT_MIN_COVER_INV
    assert R.dict_placed(hot) == len(hot)  # every one finds a slot
    assert (h["w_n"], h["w_total"]) == (len(hot) + cl["unicode"], len(hot) + cl["unicode"] + cl["spills"])


def test_long_refs_oracle():
    """The Kelvin word is in the oracles' tables once, with the summed count;
    so is the word with the NUL byte."""
    case = G.case("long_refs")
    want = case.claims["expected"]
    got, tokens = coracle.count(case.text)
    assert dict(got) == want and len(got) == len(want) and tokens == sum(want.values())
    py = pyoracle.count_words(case.text)
    assert {w.encode("utf-8"): c for w, c in py.items()} == want
    assert want[case.claims["kelvin"]] == 8 and sum(1 for w, _ in got if w == case.claims["kelvin"]) == 1
    fig = case.figures
    # both kinds of reference reach the long table for the Kelvin and the NUL word
    for word in (case.claims["kelvin"], b"a\0k", b"kixteen_bytes_wdx"):
        spell = [t for t, low in zip(fig.distinct_tokens, fig.low) if low == word]
        assert any(max(t) < 0x80 for t in spell) and any(max(t) >= 0x80 for t in spell)
        assert word in fig.long_words
    assert b"kixteen_bytes_wd" in fig.short_words and fig.u_short_n == 1
    a, b = sorted(w for w in fig.long_words if w.startswith(b"abcdefghij"))
    assert len(a) == len(b) and a[:-1] == b[:-1] and a[-1] != b[-1]


def test_pool_ladder_second_run_keeps_what_the_first_learnt():
    case = G.case("pool_ladder")
    eng = G.EngineModel()
    first = eng.run(case.figures)
    learnt = eng.next_cold_cap
    second = eng.run(case.figures)
    print("pool_ladder: %s, learnt cold cap %d, second run %s" % (G.describe(first), learnt, G.describe(second)))
    assert [h["overflow"] for h, _ in first] == [G.OVF_POOL | G.OVF_W, G.OVF_W, 0]
    assert learnt == G.cold_cap_for(first[-1][1], first[-1][0]) > G.initial_caps(case.figures.n)["cold"]
    assert len(second) == 1 and second[0][0]["overflow"] == 0 and second[0][1]["cold"] == learnt == first[-1][1]["cold"]
    rows = case.figures.rows_of
    assert set(rows.tolist()) == {8, 9}


def test_w_alone_details():
    """At most spill_cap spills a workgroup, more than w_cap together; a second
    count on the same engine shows next_cold_cap alone: no OVF_POOL ever grew
    the regions, what the spills taught does (64 -> 66, allocated as 72)."""
    case = G.case("w_alone")
    fig = case.figures
    assert set(fig.rows_of.tolist()) == {1, 2} and fig.n_total == 1
    caps = G.realloc_sized(G.initial_caps(fig.n))
    spills = fig.spills_per_wg(caps["cold"])
    assert spills.max() == 2 * (C.PAY // 2) - 16 <= caps["spill"] and spills.sum() > caps["w"]
    eng = G.EngineModel()
    first = eng.run(fig)
    assert [c["cold"] for _, c in first] == [64, 64] and eng.next_cold_cap == 66
    second = eng.run(fig)
    assert len(second) == 1 and second[0][0]["overflow"] == 0 and second[0][1]["cold"] == 72
    assert second[0][0]["spill_need"] == 2 * (C.PAY // 2) - 72 // C.QF_MAX


def test_ladder_all_exceeds_every_capacity_it_claims():
    case = G.case("ladder_all")
    fig = case.figures
    caps = G.realloc_sized(G.initial_caps(fig.n))
    needs = needs_against_caps(fig, caps)
    for k, (need, cap) in needs.items():
        print("ladder_all: %-6s needs %9d of %9d" % (k, need, cap))
        assert need > cap
    part = np.bincount(fig.short_part, minlength=C.NB)
    assert part[case.claims["part"]] > C.SPLIT_MIN and caps["split_k"] == 0
    ladder = G.ladder_of(case)
    union = 0
    for h, _ in ladder:
        union |= h["overflow"]
    print("ladder_all: %d retries of %d: %s" % (len(ladder) - 1, C.GROW_RETRIES, [G.mask_names(h["overflow"]) for h, _ in ladder]))
    assert union == case.claims["union"] and case.nodict
