"""No GPU: the build contract of every row of neupan_amd.build.LIBRARIES -- what each library declares, binds and exports, what
it is built from and how, when it is rebuilt, that a row lists every file its sources include, and that the units of a row reach
each other through csrc/launch.h alone."""
import itertools
import os
import re
import subprocess

import pytest

from neupan_amd import _lib, _lib_grid, _lib_train, build as b

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS = list(b.LIBRARIES)
BINDINGS = {"main": _lib, "train": _lib_train, "grid": _lib_grid}
# the exports of the two small libraries by name; the main header's are too many to repeat here
NAMES = {"train": {"npa_dune_train_last_error", "npa_dune_train_param_count", "npa_dune_train_steps"},
         "grid": {"npa_grid_scan", "npa_grid_clearance", "npa_grid_last_error"}}
# what the main library exports besides its header's names: the diagnostics that tests/ and tests/tools/ read through ctypes,
# declared under default visibility at the end of csrc/launch.h
HELPERS = {"npa_qp_shmem_bytes_path", "npa_group_begin_merged", "npa_group_iter_merged", "npa_dbg_group_merged_launches",
           "npa_dbg_pack_image", "npa_dbg_sel_prof"}
SEL_PROF_ONLY = {"npa_dbg_sel_prof"}            # defined in the -DNPA_SEL_PROF variant alone (tests/tools/select_phase_cycles.py)


def code(path):
    """the file without its comments"""
    return re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S))


def declared(name):
    """the npa_* functions the row's own header declares"""
    return set(re.findall(r"\b(npa_\w+)\s*\(", code(os.path.join(ROOT, "include", b.LIBRARIES[name].headers[0]))))


def file_scope(path):
    """the file's text outside every function and class body (a body becomes `{}`): no comments, no preprocessor lines, string
    and character literals emptied; the braces of `namespace ... {` and `extern "C" {` are not bodies"""
    txt = re.sub(r"^[ \t]*#(?:[^\n]*\\\n)*[^\n]*", "", code(path), flags=re.M)
    txt = txt.replace('extern "C"', "extern C")
    txt = re.sub(r"'(?:\\.|[^'\\\n])'", "' '", re.sub(r'"(?:\\.|[^"\\\n])*"', '""', txt))
    out, stack, start = [], [], 0                     # stack: True for a body; start: where the current statement began
    for i, ch in enumerate(txt):
        inside = any(stack)
        if ch == "{":
            head = txt[start:i]
            stack.append(not re.search(r"(?:\bnamespace\b[\w\s:]*|\bextern C\s*)$", head))
            if not inside:
                out.append("{" if stack[-1] else " ")
            start = i + 1
        elif ch == "}":
            body = stack.pop()
            if not any(stack):
                out.append("}" if body else " ")
            start = i + 1
        else:
            if ch == ";":
                start = i + 1
            if not inside:
                out.append(ch)
    assert not stack, path
    return "".join(out).replace("extern C", 'extern "C"')


def test_the_table_is_what_it_was():
    assert ROWS == ["main", "train", "grid"] and set(BINDINGS) == set(ROWS)
    assert b.SOURCES == ["dune.hip", "nrmp_qp.hip", "frontend.hip", "dune_labels.hip", "c_api.hip", "create.hip", "pack_image.hip",
                         "serve_group.hip", "ingest.hip", "clearance.hip", "world.hip", "behave.hip", "cycle.hip", "lon.hip",
                         "curves.hip"]
    assert b.TRAIN_SOURCES == ["dune_train.hip"] and b.GRID_SOURCES == ["grid.hip"]
    assert [os.path.basename(p) for p in (b.LIB, b.TRAIN_LIB, b.GRID_LIB)] == ["libneupan_amd.so", "libneupan_amd_train.so",
                                                                              "libneupan_amd_grid.so"]
    assert [b.LIBRARIES[k].sources for k in ROWS] == [b.SOURCES, b.TRAIN_SOURCES, b.GRID_SOURCES]
    assert [b.LIBRARIES[k].lib for k in ROWS] == [b.LIB, b.TRAIN_LIB, b.GRID_LIB]
    assert [BINDINGS[k].LIB_PATH for k in ("train", "grid")] == [b.TRAIN_LIB, b.GRID_LIB]
    for x, y in itertools.combinations(ROWS, 2):                 # a source is one library's
        assert not set(b.LIBRARIES[x].sources) & set(b.LIBRARIES[y].sources), (x, y)


@pytest.mark.parametrize("name", ROWS)
def test_symbols_declared_bound_and_exported(name):
    """header == SYMBOLS == what the loaded library gives a prototype; the dynamic exports are these names and nothing else --
    for the main library these and HELPERS, by name"""
    names, mod, row = declared(name), BINDINGS[name], b.LIBRARIES[name]
    b.build_library(name, force=False, verbose=False)
    assert names == set(mod.SYMBOLS) == NAMES.get(name, names) and len(names) >= (12 if name == "main" else 3)
    out = subprocess.run(["nm", "-D", "--defined-only", row.lib], stdout=subprocess.PIPE, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if " T " in ln and ln.split()[-1].startswith("npa_")}
    want = names | (HELPERS - SEL_PROF_ONLY) if name == "main" else names
    assert exported == want, exported ^ want
    lib = mod.load()
    for n in names:
        assert getattr(lib, n).argtypes is not None, n


def test_the_helpers_are_the_default_visibility_block_of_launch_h():
    txt = code(os.path.join(b.CSRC, "launch.h"))
    inner, block = txt.split("#pragma GCC visibility push(default)")
    block, rest = block.split("#pragma GCC visibility pop")
    assert set(re.findall(r"\b(npa_\w+)\s*\(", block)) == HELPERS and 'extern "C"' in block
    assert 'extern "C"' not in inner and "npa_" not in rest
    assert "-fvisibility=hidden" in b.FLAGS
    for row in b.LIBRARIES.values():                 # the exports: between push(default) and pop of the row's own header
        hdr = code(os.path.join(ROOT, "include", row.headers[0]))
        assert hdr.count("#pragma GCC visibility push(default)") == 1 and hdr.count("#pragma GCC visibility pop") == 1
        before, after = hdr.split("#pragma GCC visibility push(default)")[0], hdr.split("#pragma GCC visibility pop")[1]
        assert not re.search(r"\bnpa_\w+\s*\(", before + after), row.headers[0]


def prototypes(scope_text):
    """the npa_* functions declared without a body in a file_scope() text (a `static` forward declaration is not one: the unit
    that holds it also holds the definition, and the compiler compares the two)"""
    return [m.group(2) for m in re.finditer(r"([^;{}]*?)\b(npa_\w+)\s*\([^;{}]*\)\s*;", scope_text) if "static" not in m.group(1).split()]


def test_no_unit_writes_a_prototype():
    """a function another unit defines is declared in a header: no .hip file of any row holds a prototype without a body"""
    for row in b.LIBRARIES.values():
        for src in row.sources:
            path = os.path.join(b.CSRC, src)
            assert not re.findall(r'^\s*extern "C"[^;{]*\)\s*;', code(path), flags=re.M), src
            assert not prototypes(file_scope(path)), src


def test_file_scope_sees_prototypes_and_only_them():
    """(the helper of the test above, on a text that has every case)"""
    import tempfile
    text = ('#define M(x) do { x; } while (0)\nnamespace {\nint npa_a(int);  // one\nstatic int f() { return npa_b(1); }\n}\n'
            'extern "C" {\nint npa_c(void);\n}\nextern "C" int npa_d(int x) { if (x) { npa_e(x); } return 0; }\n'
            'struct S { int npa_f(int); };\nconst char* s = "npa_g(1);";\nhipError_t npa_h(const float* a,\n    int b);\n'
            'static int npa_i(int);\n')
    with tempfile.NamedTemporaryFile("w", suffix=".hip") as f:
        f.write(text)
        f.flush()
        assert prototypes(file_scope(f.name)) == ["npa_a", "npa_c", "npa_h"]


def test_every_cross_unit_function_is_declared_once_in_launch_h():
    """every non-static npa_* function that one unit of the main library defines and another names is declared in csrc/launch.h
    or in the public header -- and launch.h declares nothing twice and nothing that no unit defines"""
    row = b.LIBRARIES["main"]
    assert "launch.h" in row.includes
    scope = {src: file_scope(os.path.join(b.CSRC, src)) for src in row.sources}
    text = {src: code(os.path.join(b.CSRC, src)) for src in row.sources}
    defined = {}
    for src, txt in scope.items():
        for m in re.finditer(r"([^;{}]*?)\b(npa_\w+)\s*\([^;{}]*\)\s*\{\}", txt):
            if not set(m.group(1).split()) & {"static", "__global__", "__device__"}:
                defined.setdefault(m.group(2), set()).add(src)
    assert len(defined) > 60 and all(len(v) == 1 for v in defined.values()), {k: v for k, v in defined.items() if len(v) > 1}
    in_launch = re.findall(r"\b(npa_\w+)\s*\(", code(os.path.join(b.CSRC, "launch.h")))
    assert len(in_launch) == len(set(in_launch)), sorted(n for n in set(in_launch) if in_launch.count(n) > 1)
    assert set(in_launch) - SEL_PROF_ONLY <= set(defined), set(in_launch) - set(defined)
    known = set(in_launch) | declared("main")
    crossing = {n for n, (src,) in ((n, tuple(v)) for n, v in defined.items())
                if any(re.search(r"\b%s\b" % n, t) for other, t in text.items() if other != src)}
    assert len(crossing) >= 30 and crossing <= known, sorted(crossing - known)
    # every unit that defines or names one of launch.h's functions includes the header itself
    for src, t in text.items():
        if any(re.search(r"\b%s\b" % n, t) for n in in_launch):
            assert re.search(r'^[ \t]*#[ \t]*include[ \t]*"launch.h"', t, flags=re.M), src


def test_symbol_tables_are_pairwise_disjoint():
    for x, y in itertools.combinations(ROWS, 2):
        assert not set(BINDINGS[x].SYMBOLS) & set(BINDINGS[y].SYMBOLS), (x, y)
    assert not [s for s in _lib.SYMBOLS if "grid" in s]


def test_main_library_keeps_its_version_and_its_size():
    from conftest import experiments_built
    b.build(force=False, verbose=False)
    version = _lib.load().npa_version()
    assert b"0.5.2" in version and b"gfx950" in version
    if not experiments_built():
        assert os.path.getsize(b.LIB) < 2 * 1024 * 1024, os.path.getsize(b.LIB)


@pytest.mark.parametrize("name", ROWS)
def test_unvalidated_compiler_is_refused_and_a_forced_build_compiles_every_unit_and_links_once(name, monkeypatch):
    """neupan_amd.build fails (not warns) on a hipcc other than the validated one unless NPA_ALLOW_UNVALIDATED=1, before any
    command runs; with it, one compile per source with the build's flags, objects under neupan_amd/_obj, one stripped link."""
    row, calls = b.LIBRARIES[name], []
    monkeypatch.setattr(b, "hipcc_version", lambda: "9.9.99999-test")
    monkeypatch.setattr(b.subprocess, "check_call", lambda cmd, *a, **k: calls.append(cmd))

    class FakeProc:                                   # (the translation units are compiled side by side: Popen + wait)
        def __init__(self, cmd, *a, **k):
            calls.append(cmd)

        def wait(self):
            return 0
    monkeypatch.setattr(b.subprocess, "Popen", FakeProc)
    monkeypatch.delenv("NPA_ALLOW_UNVALIDATED", raising=False)
    with pytest.raises(b.UnvalidatedCompiler):
        b.build_library(name, force=True, verbose=False)
    assert not calls
    monkeypatch.setenv("NPA_ALLOW_UNVALIDATED", "1")
    assert {"main": b.build, "train": b.build_train, "grid": b.build_grid}[name](force=True, verbose=False) == row.lib
    assert len(calls) == len(row.sources) + 1          # every source compiled, one link
    objs = [os.path.join(ROOT, "neupan_amd", "_obj", src.replace(".hip", ".o")) for src in row.sources]
    for cmd, src, obj in zip(calls, row.sources, objs):
        assert all(f in cmd for f in b.FLAGS) and os.path.join("neupan_amd", "_obj") in cmd[-1]
        assert cmd == [b.hipcc_path(), *b.FLAGS, '-DNPA_HIPCC_VERSION="9.9.99999-test"', "-c",
                       os.path.join(ROOT, "neupan_amd", "csrc", src), "-o", obj]
    assert "-Wl,--strip-all" in calls[-1] and calls[-1][-1] == row.lib
    assert calls[-1] == [b.hipcc_path(), "--offload-arch=gfx950", "-shared", "-fPIC", "-Wl,--strip-all", *objs, "-o", row.lib]


def _closure(name):
    """every file the row's sources reach through #include "...", resolved relative to the including file"""
    todo = [os.path.join(b.CSRC, src) for src in b.LIBRARIES[name].sources]
    seen = set()
    while todo:
        path = os.path.normpath(todo.pop())
        if path in seen:
            continue
        seen.add(path)
        for inc in re.findall(r'^[ \t]*#[ \t]*include[ \t]*"([^"]+)"', open(path).read(), flags=re.M):
            todo.append(os.path.join(os.path.dirname(path), inc))
    return seen


@pytest.mark.parametrize("name", ROWS)
def test_a_row_lists_every_file_its_sources_include(name):
    listed = {os.path.normpath(f) for f in b.LIBRARIES[name].files()}
    reached = _closure(name)
    assert len(reached) > len(b.LIBRARIES[name].sources)         # (the walk found includes at all)
    assert reached <= listed, sorted(reached - listed)
    assert all(os.path.exists(f) for f in listed), sorted(f for f in listed if not os.path.exists(f))


@pytest.mark.parametrize("touched, stale", [("csrc/grid.hip", {"grid"}), ("csrc/scan_beam.h", {"main", "grid"}),
                                            ("csrc/handle.h", {"main"}), ("csrc/dune_train.hip", {"train"}),
                                            ("csrc/aset_reduce.h", set()), ("_obj/dune.o", set()),
                                            ("../include/neupan_amd_grid.h", {"grid"}),
                                            ("../include/neupan_amd.h", {"main", "train", "grid"}),
                                            ("csrc/launch.h", {"main"})])
def test_needs_build_follows_the_row_and_nothing_else(touched, stale, monkeypatch):
    """a library is stale when a file of ITS row is newer -- not whatever lies in csrc/ -- or when it is missing (times and
    existence are faked: the tree is not touched)"""
    outputs = {os.path.normpath(row.lib) for row in b.LIBRARIES.values()}
    newer = os.path.normpath(os.path.join(ROOT, "neupan_amd", touched))
    mtime = lambda p: 3.0 if os.path.normpath(p) == newer else (2.0 if os.path.normpath(p) in outputs else 1.0)
    monkeypatch.setattr(b.os.path, "getmtime", mtime)
    monkeypatch.setattr(b.os.path, "exists", lambda p: True)
    assert {k for k in ROWS if b.needs_build(k)} == stale
    monkeypatch.setattr(b.os.path, "exists", lambda p: os.path.normpath(p) != os.path.normpath(b.GRID_LIB))
    assert {k for k in ROWS if b.needs_build(k)} == stale | {"grid"}
