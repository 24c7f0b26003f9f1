"""The C-ABI library loads and exports every symbol include/*.h declares (no compute calls: no GPU here)."""
import ctypes
import glob
import os
import re
import multi_orb_slam_amd as m

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_functions():
    names = []
    for h in sorted(glob.glob(os.path.join(ROOT, "include", "*.h"))):
        src = re.sub(r"/\*.*?\*/", "", open(h).read(), flags=re.S)
        names += re.findall(r"\b(orb[xmfv]?_[a-z0-9_]+)\s*\(", src)
    return sorted(set(names))


def test_library_exports_every_declared_symbol():
    lib = ctypes.CDLL(m.LIB_PATH)
    fns = declared_functions()
    assert len(fns) >= 80
    for f in fns:
        assert hasattr(lib, f), f


def test_no_device_is_a_loud_error_not_a_fallback():
    # in the CPU container there is no GPU: every handle constructor must fail with ORB_E_NO_DEVICE
    import torch
    if torch.cuda.is_available():
        return
    for ctor in (lambda: m.Matcher(), lambda: m.Extractor(m.ExtractorParams(), 640, 480)):
        try:
            ctor()
        except m.OrbError as e:
            assert e.code == -4 and "no CPU path" in str(e)
        else:
            raise AssertionError("constructor succeeded without a GPU")


def test_keypoint_and_query_layouts():
    assert m.KP_DTYPE.itemsize == 28 and m.QUERY_DTYPE.itemsize == 68
    assert [m.KP_DTYPE.fields[k][1] for k in ("x", "y", "size", "angle", "response", "octave", "class_id")] == \
        [0, 4, 8, 12, 16, 20, 24]


def test_product_never_imports_the_oracle():
    pkg = os.path.join(ROOT, "multi_orb_slam_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".h", ".hip", ".cpp", ".cc")) or f == "Makefile":
                txt = open(os.path.join(dirpath, f), errors="replace").read()
                assert "oracle/" not in txt and "import oracle" not in txt and "liborb_oracle" not in txt, f


def test_resolve_form_codes_of_the_binding_are_those_of_the_header():
    """matcher.FORM_* (what Matcher.last_resolve_form() is read with) against ORBM_FORM_* of include/orb_debug.h: every code, by name."""
    from multi_orb_slam_amd import matcher
    src = open(os.path.join(ROOT, "include", "orb_debug.h")).read()
    header = {name: int(val) for name, val in re.findall(r"#define ORBM_FORM_([A-Z0-9_]+)\s+(\d+)", src)}
    binding = {k[len("FORM_"):]: v for k, v in vars(matcher).items() if k.startswith("FORM_")}
    assert len(header) == 10 and len(set(header.values())) == 10
    assert binding == header


def test_last_join_report_of_the_binding_is_the_one_of_the_header():
    """BowSearch.last_join() (what the BoW boundary tests assert their form with) against orbv_debug_last_join of include/orb_debug.h: the
    declaration, its four fields in the order the binding names them, the export and the binding's argument list."""
    import inspect
    from multi_orb_slam_amd import _lib, vocabulary
    src = open(os.path.join(ROOT, "include", "orb_debug.h")).read()
    decl = re.search(r"/\*((?:(?!\*/).)*)\*/\s*int orbv_debug_last_join\(const orbv_workspace\* w, int\* out4\);", src, re.S)
    assert decl, "orbv_debug_last_join is not declared as (const orbv_workspace*, int* out4)"
    fields = re.search(r"\{(.*?)\}", decl.group(1), re.S).group(1)
    order = [fields.index(k) for k in ("waves per vocabulary node", "largest node of side B", "lds_cand", "mode")]
    assert order == sorted(order) and fields.count(",") >= 3
    lib = _lib.lib()
    assert hasattr(lib, "orbv_debug_last_join") and len(lib.orbv_debug_last_join.argtypes) == 2
    doc = inspect.getdoc(vocabulary.BowSearch.last_join)
    assert "orbv_debug_last_join" in doc and [doc.index(k) for k in ("waves per node", "largest node", "staged in LDS", "mode")] == sorted(
        doc.index(k) for k in ("waves per node", "largest node", "staged in LDS", "mode"))
    assert "(ctypes.c_int * 4)" in inspect.getsource(vocabulary.BowSearch.last_join).replace("C.c_int", "ctypes.c_int")


def test_keyframe_build_and_database_query_reports_of_the_binding_are_those_of_the_header():
    """BowSearch.last_keyframe_build() and KeyFrameDatabase.last_query() (what the vocabulary and database boundary tests assert their
    forms with) against orbv_debug_last_keyframe_build / orbv_debug_last_db_query of include/orb_debug.h: the declarations, the fields in
    the order the bindings name them, the form codes, the exports and the bindings' argument lists."""
    import inspect
    from multi_orb_slam_amd import _lib, vocabulary
    src = open(os.path.join(ROOT, "include", "orb_debug.h")).read()
    lib = _lib.lib()
    for fn, sig, header_keys, method, doc_keys, n in (
            ("orbv_debug_last_keyframe_build", r"\(const orbv_workspace\* w, int\* out5\)", ("bins", "chunks of 1024", "FeatureVector\n * nodes", "largest node", "items"),
             vocabulary.BowSearch.last_keyframe_build, ("bins", "chunks of 1024", "FeatureVector nodes", "largest node", "items"), 5),
            ("orbv_debug_last_db_query", r"\(const orbv_database\* db, int\* out4\)", ("form of k_db_query", "entries per workgroup", "workgroups per query", "queries"),
             vocabulary.KeyFrameDatabase.last_query, ("form", "entries per workgroup", "workgroups per query", "queries"), 4)):
        decl = re.search(r"/\*((?:(?!\*/).)*)\*/\s*(?:#define[^\n]*\n)*int %s%s;" % (fn, sig), src, re.S)
        assert decl, fn
        fields = re.search(r"\{(.*?)\}", decl.group(1), re.S).group(1)
        order = [fields.index(k) for k in header_keys]
        assert order == sorted(order), fn
        assert hasattr(lib, fn) and len(getattr(lib, fn).argtypes) == 2
        doc = inspect.getdoc(method)
        assert fn in doc and [doc.index(k) for k in doc_keys] == sorted(doc.index(k) for k in doc_keys)
        assert "(ctypes.c_int * %d)" % n in inspect.getsource(method).replace("C.c_int", "ctypes.c_int")
    header = {name: int(val) for name, val in re.findall(r"#define ORBV_DB_FORM_([A-Z]+)\s+(\d+)", src)}
    assert header == {"LDS": vocabulary.DB_FORM_LDS, "GLOBAL": vocabulary.DB_FORM_GLOBAL} and len(set(header.values())) == 2
