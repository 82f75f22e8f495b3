"""CPU: the one home of the buffers of the calls over the result
(map-oxidize_amd/csrc/mox_result.hip): every DevBuf of the engine is freed in
exactly one place, the helpers are defined once, the scratch layouts go through
Carve (mox_carve.h), and the build plan of the objects that are no call over
the result.  No GPU code runs here."""
import itertools
import re

from srcpins import CHECK_FLAGS, HC_FLAGS, KERNEL_FLAGS, LIBS, _read, make_plan

CSRC = ("map-oxidize_amd", "csrc")
OPS = ("bsort", "topk", "text", "accum", "lookup", "filter", "rank", "rekey", "find", "hist", "join")
# the DevBufs that are no operator's: the exchange's and the gather's, freed by mox_engine_destroy itself
ELSEWHERE = {"x_send_short", "x_send_blob", "x_recv_short", "x_recv_blob", "hx_send", "hx_recv", "g_counts", "g_offs", "g_bytes", "g_recv"}


def engine_devbufs():
    """Every DevBuf of struct mox_engine, arrays expanded: 'a_tab[0]', 'f_tab[1][2]', 'k_tmp', ..."""
    host = _read(*CSRC, "mox_host.h")
    body = host.split("struct mox_engine {")[1].split("\nnamespace mox_host {")[0]
    out = []
    for decl in re.findall(r"^  DevBuf ([^;]+);", body, re.M):
        for item in decl.split(","):
            name, dims = re.match(r"\s*(\w+)((?:\[\d+\])*)\s*$", item).groups()
            sizes = [int(d) for d in re.findall(r"\[(\d+)\]", dims)]
            for idx in itertools.product(*[range(k) for k in sizes]):
                out.append(name + "".join("[%d]" % i for i in idx))
    return out


def test_result_free_frees_every_operator_buffer_once():
    bufs = engine_devbufs()
    assert len(bufs) == len(set(bufs)) and {"k_tmp", "a_tab[2]", "f_tab[1][2]", "tx_pin[1]", "h_rmax", "h_bsort", "hg_pin"} <= set(bufs)
    assert ELSEWHERE <= set(bufs)
    src = _read(*CSRC, "mox_result.hip")
    body = src.split("void result_free(mox_engine* e) {")[1].split("\n}\n")[0]
    freed = re.findall(r"&e->(\w+(?:\[\d+\])*)", body)
    assert sorted(freed) == sorted(b for b in bufs if b.split("[")[0] not in ELSEWHERE)  # each one, once
    # the device ones through free_bufs, the pinned ones through hipHostFree, the text's events destroyed
    dev, pinned = body.split("free_bufs({")[1].split("});")[0], body.split("for (DevBuf* b : {")[1].split("})")[0]
    assert set(re.findall(r"&e->(\w+)", pinned)) == {"h_bsort", "tx_pin", "l_pin", "h_rmax", "fd_pin", "hg_pin"}
    assert not set(re.findall(r"&e->(\w+)", dev)) & set(re.findall(r"&e->(\w+)", pinned))
    assert "hipHostFree(b->p)" in body and "hipEventDestroy(ev)" in body and "e->tx_ev" in body
    # every pinned DevBuf is grown by grow_pinned and by nothing else
    for name in ("h_bsort", "tx_pin", "l_pin", "h_rmax", "fd_pin", "hg_pin"):
        grown = [f for f in OPS if "grow_pinned(e->%s" % name in _read(*CSRC, "mox_%s.hip" % f)]
        assert len(grown) == 1, (name, grown)
    # the others stay where they were: each of them in mox_engine_destroy, none here
    destroy = _read(*CSRC, "mox_engine.hip").split("void mox_engine_destroy(mox_engine* e) {")[1].split("\n}\n")[0]
    assert set(re.findall(r"&e->(\w+)", destroy)) == ELSEWHERE
    assert destroy.count("result_free(e);") == 1 and destroy.count("xplan_free(e);") == 1
    # no other free function over the engine is left
    host = _read(*CSRC, "mox_host.h")
    assert re.findall(r"(\w+)_free\(mox_engine", host) == ["result", "xplan"]
    for f in OPS + ("engine", "multi"):
        assert not re.search(r"^void \w+_free\(mox_engine", _read(*CSRC, "mox_%s.hip" % f).replace("void xplan_free(", ""), re.M), f


def test_the_helpers_have_one_home():
    src, host = _read(*CSRC, "mox_result.hip"), _read(*CSRC, "mox_host.h")
    section = host.split("// ---- mox_result.hip")[1].split("// ---- ")[0]
    for name in ("grow_dev", "grow_pinned", "free_bufs", "table_reserve", "table_other_set", "res_point_at", "grid_cap", "test_fail_hook",
                 "result_free"):
        assert len(re.findall(r"^[\w:*]+\*? %s\(" % name, src, re.M)) == 1, name
        assert re.search(r"^[\w:*]+\*? %s\(" % name, section, re.M), name
        for f in OPS + ("engine", "multi"):
            assert not re.search(r"^[\w:*]+\*? %s\(" % name, _read(*CSRC, "mox_%s.hip" % f), re.M), (name, f)
    assert "mox_result.hip" in host.split("#pragma once")[0] and "__global__" not in src and "hipLaunchKernelGGL" not in src
    # a table in an operator's buffers is no pass table and no exchanged one: res_point_at says so, its callers do not
    body = src.split("void res_point_at(")[1].split("\n}\n")[0]
    assert "r.pass = false;" in body and "r.exchanged = false;" in body
    assert not re.search(r"\b(sorted|ranked|folded)\b", body)
    callers = 0
    for f in OPS:
        text = _read(*CSRC, "mox_%s.hip" % f)
        for m in re.finditer(r"res_point_at\((\w+),[^;]*;\n((?:.*\n){2})", text):
            callers += 1
            assert not re.search(r"\.(pass|exchanged) = ", m.group(2)), (f, m.group(0))
    assert callers == 4  # filter, join, rank, acc_as_result
    # the n <= 1 path of the ranking installs no table and keeps its own lines
    assert "    e->res.pass = false;\n    e->res.exchanged = false;\n    e->res.ranked = true;\n" in _read(*CSRC, "mox_rank.hip")


def test_scratch_layouts_go_through_carve():
    carve = _read(*CSRC, "mox_carve.h")
    assert re.findall(r"#include <(\w+)>", carve) == ["cstddef", "cstdint"] and '#include "' not in carve and "hip" not in carve.split("#pragma once")[1]
    assert "size_t align = 256" in carve
    laid_out = {"bsort": ["s_tmp"], "topk": ["k_tmp"], "lookup": ["l_tmp"], "find": ["fd_tmp"], "filter": ["f_tmp"], "join": ["j_tmp"],
                "rank": ["r_tmp"], "hist": ["hg_tmp", "hg_out"]}
    for f in OPS:
        text = re.sub(r"//.*", "", _read(*CSRC, "mox_%s.hip" % f))
        assert not re.search(r"\+ 255\) ?&|& ?~\(?\(?size_t\)?7|\bup\(", text), f  # no rounding by hand
        assert not re.search(r";\s*\w+ \+= \w+_b;", text), f  # no pointer walk over byte sizes
        for buf in laid_out.get(f, []):
            assert "grow_dev(e->%s" % buf not in text.replace("grow_dev(e->s_tmp, need)", ""), (f, buf)
            if buf != "s_tmp":
                assert text.count("carve_dev(e->%s, [&](Carve& c) {" % buf) == 1, (f, buf)
    bsort = _read(*CSRC, "mox_bsort.hip")
    assert "auto layout = [&](Carve& c) {" in bsort and bsort.count("layout(") == 2  # one function: the sizing and the placing
    # the alignment table of the sort stays: it also covers the borrowed arrays
    assert '{"tick", s.tick, 8}, {"status", s.status, 8}, {"gh", s.gh, 8}, {"gs", s.gs, 8}' in bsort


def test_build_plan_of_the_other_objects():
    objs, libs = make_plan()
    assert objs["mox_kernels.o"] == ("mox_kernels.hip", KERNEL_FLAGS)
    assert objs["mox_kernels_check.o"] == ("mox_kernels.hip", KERNEL_FLAGS + CHECK_FLAGS)
    assert objs["mox_kernels_hc.o"] == ("mox_kernels.hip", KERNEL_FLAGS + HC_FLAGS)
    assert objs["mox_engine.o"] == ("mox_engine.hip", []) and objs["mox_multi.o"] == ("mox_multi.hip", [])
    assert objs["mox_engine_check.o"] == ("mox_engine.hip", CHECK_FLAGS)
    assert objs["mox_engine_hc.o"] == ("mox_engine.hip", HC_FLAGS) and objs["mox_multi_hc.o"] == ("mox_multi.hip", HC_FLAGS)
    assert objs["mox_result.o"] == ("mox_result.hip", [])  # host code: no KERNEL_FLAGS; hashes nothing: one object
    assert not [o for o in objs if o.startswith("mox_result_") or o == "mox_multi_check.o"]
    hc_ops = ("accum", "lookup", "rekey", "join")
    assert sorted(objs) == sorted(["mox_kernels.o", "mox_kernels_check.o", "mox_kernels_hc.o", "mox_engine.o", "mox_engine_check.o",
                                   "mox_engine_hc.o", "mox_multi.o", "mox_multi_hc.o", "mox_result.o"] +
                                  ["mox_%s.o" % op for op in OPS] + ["mox_%s_hc.o" % op for op in hc_ops])
    assert set(libs) == set(LIBS)
    ops = lambda hc: ["mox_%s%s.o" % (op, "_hc" if hc and op in hc_ops else "") for op in OPS]
    tail = ["mox_result.o", "mox_table.o"]
    assert libs["libmox.so"] == ["mox_kernels.o", "mox_engine.o", "mox_multi.o"] + ops(False) + tail
    assert libs["libmox_check.so"] == ["mox_kernels_check.o", "mox_engine_check.o", "mox_multi.o"] + ops(False) + tail
    assert libs["libmox_hc.so"] == ["mox_kernels_hc.o", "mox_engine_hc.o", "mox_multi_hc.o"] + ops(True) + tail
