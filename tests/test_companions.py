"""The companion libraries' plumbing, pinned: build.COMPANIONS and binding.COMPANIONS describe the same seven libraries, and what the
named wrappers around the two tables expose - library paths, export lists, ctypes prototypes, the Scene.draw_* signatures, build_all()'s
order, what each example links - is what tests/golden/companion_abi.json recorded before the tables existed.

`python tests/test_companions.py --record` rewrites that file from the tree it runs in (it builds first)."""
import inspect
import json
import os
import subprocess
import sys

NAMES = ["trace", "split", "path", "gloss", "virtual", "rough", "highlight"]
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "companion_abi.json")


def _svgf_needed(path):
    out = subprocess.run(["readelf", "-d", path], stdout=subprocess.PIPE, text=True, check=True).stdout
    return sorted(ln.split("[")[1].split("]")[0] for ln in out.splitlines() if "(NEEDED)" in ln and "[libsvgf_" in ln)


def snapshot(pkg, root):
    """Everything the golden file holds, read from the package as it is (paths as file names: a checkout may lie anywhere)."""
    B, bld = pkg.binding, pkg.build
    tname = lambda t: None if t is None else t.__name__      # noqa: E731
    snap = {"functions": {}, "signatures": {}, "names": {}, "exports": {}, "sources": {}}
    for n in NAMES:
        lib = getattr(B, f"load_{n}_library")()
        for sym in getattr(B, f"{n.upper()}_EXPORTS"):
            f = getattr(lib, sym)
            snap["functions"][sym] = {"argtypes": None if f.argtypes is None else [tname(t) for t in f.argtypes], "restype": tname(f.restype)}
        snap["exports"][f"{n.upper()}_EXPORTS"] = list(getattr(B, f"{n.upper()}_EXPORTS"))
        snap["sources"][f"{n.upper()}_SOURCES"] = list(getattr(bld, f"{n.upper()}_SOURCES"))
        snap["names"][f"LIB_{n.upper()}"] = os.path.relpath(getattr(bld, f"LIB_{n.upper()}"), root)
        snap["names"][f"LIB_{n.upper()}_PATH"] = os.path.relpath(getattr(B, f"LIB_{n.upper()}_PATH"), root)
    for m in sorted(k for k in vars(pkg.Scene) if k.startswith("draw") and k != "draw_planar"):
        snap["signatures"][f"Scene.{m}"] = str(inspect.signature(getattr(pkg.Scene, m)))
    for cls in (pkg.GlossTable, pkg.RoughTable):
        snap["signatures"][f"{cls.__name__}.__init__"] = str(inspect.signature(cls.__init__))
    snap["build_all"] = [os.path.relpath(p, root) for p in bld.build_all()]
    bld.build_examples()
    ex = os.path.join(root, "examples")
    snap["example_needed"] = {e[:-4]: _svgf_needed(os.path.join(ex, e[:-4])) for e in sorted(os.listdir(ex)) if e.endswith(".cpp")}
    return snap


def test_the_two_tables_name_the_same_seven_libraries_in_the_order_they_were_added(pkg):
    assert [c.name for c in pkg.build.COMPANIONS] == NAMES == [c.name for c in pkg.binding.COMPANIONS]
    assert [pkg.build.companion_path(n) for n in NAMES] == [pkg.binding.companion_path(n) for n in NAMES] == pkg.build.build_all()[1:]
    assert pkg.build.build_all()[0] == pkg.build.LIB == pkg.binding.LIB_PATH


def test_prototypes_signatures_names_and_links_are_what_they_were_before_the_tables(pkg):
    from conftest import ROOT
    want, got = json.load(open(GOLDEN)), snapshot(pkg, ROOT)
    assert len(want["signatures"]) == 16 and len(want["build_all"]) == 8 and len(want["functions"]) == sum(len(v) for v in want["exports"].values())
    for section in want:
        assert set(got[section]) == set(want[section]) if isinstance(want[section], dict) else True, section
        for key in (want[section] if isinstance(want[section], dict) else ()):
            assert got[section][key] == want[section][key], (section, key)
    assert got == want


if __name__ == "__main__" and sys.argv[1:] == ["--record"]:
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from conftest import ROOT, ge
    ge.build()
    json.dump(snapshot(ge.load_package(), ROOT), open(GOLDEN, "w"), indent=1, sort_keys=True)
    print("wrote", GOLDEN)
