"""No GPU: the build contract of every row of neupan_amd.build.LIBRARIES -- what each library declares, binds and exports, what
it is built from and how, when it is rebuilt, and that a row lists every file its sources include."""
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


def declared(name):
    """the npa_* functions the row's own header declares (comments taken out first)"""
    txt = open(os.path.join(ROOT, "include", b.LIBRARIES[name].headers[0])).read()
    txt = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", txt, flags=re.S))
    return set(re.findall(r"\b(npa_\w+)\s*\(", txt))


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
    """header == SYMBOLS == what the loaded library gives a prototype; the dynamic exports are these names -- for the main
    library these and the npa_* helpers its translation units call each other through, which no header declares"""
    names, mod, row = declared(name), BINDINGS[name], b.LIBRARIES[name]
    b.build_library(name, force=False, verbose=False)
    assert names == set(mod.SYMBOLS) == NAMES.get(name, names) and len(names) >= (12 if name == "main" else 3)
    out = subprocess.run(["nm", "-D", "--defined-only", row.lib], stdout=subprocess.PIPE, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if " T " in ln and ln.split()[-1].startswith("npa_")}
    assert exported >= names if name == "main" else exported == names, exported ^ names
    lib = mod.load()
    for n in names:
        assert getattr(lib, n).argtypes is not None, n


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
                                            ("../include/neupan_amd.h", {"main", "train", "grid"})])
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
