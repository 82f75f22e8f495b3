"""Helpers of the CPU tests that pin source text (tests/test_*_abi.py): reading
a file of the repository, C declarations without comments, the fields of a
typedef'd struct, and the build plan of the Makefile."""
import functools
import os
import re
import shlex
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

LIBS = ("libmox.so", "libmox_check.so", "libmox_hc.so")
KERNEL_FLAGS = ["-mllvm", "-amdgpu-sched-strategy=max-memory-clause"]
CHECK_FLAGS = ["-DMOX_CHECK"]
HC_FLAGS = ["-DMOX_HASH_COLLIDE", "-DMOX_CHECK"]


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def code_only(src):
    return re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", src, flags=re.S))


def struct_fields(src, name):
    m = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), src)
    assert m, name
    out = []
    for decl in m.group(1).split(";"):
        decl = decl.strip()
        if not decl:
            continue
        typ, rest = re.match(r"((?:const )?[a-z0-9_]+\*?) (.*)", decl).groups()
        for field in rest.split(","):
            out.append((typ, field.strip()))
    return out


@functools.lru_cache(maxsize=None)
def make_plan():
    """What `make all` would run, from a dry run (nothing is built): (objs, libs).
    objs: object file name -> (source file name, the variant flags of its compile
    command: KERNEL_FLAGS, then -D options, in command order); libs: library file
    name -> the object file names on its link line, in order."""
    r = subprocess.run(["make", "-n", "-B", "all"], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    objs, libs = {}, {}
    for line in r.stdout.splitlines():
        words = shlex.split(line)
        if "-shared" in words and words[0].endswith("hipcc"):
            lib = os.path.basename(words[words.index("-o") + 1])
            assert lib not in libs, lib
            libs[lib] = [os.path.basename(w) for w in words if w.endswith(".o")]
        elif "-c" in words and words[0].endswith("hipcc"):
            obj = os.path.basename(words[words.index("-o") + 1])
            assert obj not in objs, obj
            flags = [w for i, w in enumerate(words) if w.startswith("-D") or w.startswith("-amdgpu-") or
                     (w == "-mllvm" and words[i + 1].startswith("-amdgpu-"))]
            objs[obj] = (os.path.basename(words[words.index("-c") + 1]), flags)
    return objs, libs


def op_objects(op, hc):
    """Asserts the build plan of the call over the result in mox_<op>.hip and
    returns it: the plain object compiled with KERNEL_FLAGS alone, exactly once
    in libmox.so and libmox_check.so; in libmox_hc.so exactly once too, as the
    _hc object (KERNEL_FLAGS and HC_FLAGS) when hc, else the plain one, and then
    no _hc object exists; never a _check object."""
    objs, libs = make_plan()
    plain, hco, src = "mox_%s.o" % op, "mox_%s_hc.o" % op, "mox_%s.hip" % op
    assert objs[plain] == (src, KERNEL_FLAGS), objs[plain]
    assert "mox_%s_check.o" % op not in objs
    if hc:
        assert objs[hco] == (src, KERNEL_FLAGS + HC_FLAGS), objs[hco]
    else:
        assert hco not in objs
    for lib in LIBS:
        want, other = (hco, plain) if hc and lib == "libmox_hc.so" else (plain, hco)
        assert libs[lib].count(want) == 1 and other not in libs[lib], (lib, libs[lib])
    return objs, libs
