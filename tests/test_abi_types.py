"""The ctypes prototypes of ecm_amd._lib against the headers under include/, type by type, and the entry-point names the package
passes against the prototype tables: one census, run once per row of ecm_amd._lib.TABLES (header -> table).  The header is the
truth: the kernels are compiled against it (csrc/common.h includes it), while the tables are written by hand.  The header and the
Python sources are read as text; only the export check opens the built library, and nothing here needs a device.

tests/test_hip_abi_calls.py is the GPU half: it checks the VALUES that ops.py hands to these prototypes."""
import ast
import ctypes as C
import importlib
import os
import re

import pytest

from conftest import ROOT

INCLUDE = os.path.join(ROOT, "include")
PACKAGE = os.path.join(ROOT, "explicit-context-mapping-for-stereo-matching_amd")

# The one table from C value types to ctypes classes.  Every pointer PARAMETER is c_void_p (ops.py passes addresses as integers),
# a `const char*` RETURN is c_char_p; any other pointer return, and any type not listed here, is unknown and fails the test.
CTYPE_OF = {
    "int": C.c_int,
    "long long": C.c_longlong,
    "float": C.c_float,
    "unsigned": C.c_uint,
    "unsigned int": C.c_uint,
    "size_t": C.c_size_t,
    "double": C.c_double,
}
_TYPE_WORDS = {"int", "long", "float", "double", "unsigned", "signed", "short", "char", "void", "size_t"}


class HeaderError(Exception):
    """A declaration that the parser cannot map; the message names it."""


def _strip(src):
    src = re.sub(r"/\*.*?\*/", " ", src, flags=re.S)
    src = re.sub(r"//[^\n]*", " ", src)
    src = re.sub(r"^[ \t]*#[^\n]*(?:\\\n[^\n]*)*", " ", src, flags=re.M)            # preprocessor lines
    return re.sub(r'extern\s+"C"\s*\{', " ", src)


def _map_type(text, where, is_return):
    """One C type (names already removed) -> ctypes class, or HeaderError naming `where`."""
    words = [w for w in re.sub(r"\*", " * ", text).split() if w != "const"]
    if "*" in words:
        base = " ".join(w for w in words if w != "*")
        if not is_return:
            if not base or any(w not in _TYPE_WORDS for w in base.split()):
                raise HeaderError(f"{where}: unknown pointee type `{text.strip()}`")
            return C.c_void_p
        if base == "char" and words.count("*") == 1:
            return C.c_char_p
        raise HeaderError(f"{where}: unknown return type `{text.strip()}`")
    key = " ".join(words)
    if key == "void" and is_return:
        return None
    if key not in CTYPE_OF:
        raise HeaderError(f"{where}: unknown type `{text.strip()}`")
    return CTYPE_OF[key]


def _param_type(text, where):
    """Drop the parameter's name: the last identifier, unless it is itself a type word (an unnamed parameter)."""
    text = text.strip()
    if not text:
        raise HeaderError(f"{where}: empty parameter")
    if "(" in text or "[" in text or "..." in text:
        raise HeaderError(f"{where}: unknown type `{text}` (function pointer, array or variadic)")
    m = re.search(r"([A-Za-z_]\w*)\s*$", text)
    if m and m.group(1) not in _TYPE_WORDS and m.group(1) != "const":
        head = text[:m.start()]
        if head.strip():                                  # `int B` -> `int`;  a lone identifier is a type we do not know
            text = head
    return _map_type(text, where, is_return=False)


def parse_header(src):
    """{name: (restype, [argtypes])} of every function declaration in `src`, in ctypes classes."""
    out = {}
    for stmt in _strip(src).split(";"):
        stmt = " ".join(stmt.replace("}", " ").split())
        if "(" not in stmt:
            if stmt:
                raise HeaderError(f"not a function declaration: `{stmt}`")
            continue
        m = re.fullmatch(r"(.*?)\b([A-Za-z_]\w*)\s*\((.*)\)", stmt)
        if not m:
            raise HeaderError(f"cannot parse the declaration `{stmt}`")
        ret, name, params = m.groups()
        if name in out:
            raise HeaderError(f"{name}: declared twice")
        res = _map_type(ret, f"{name} (return)", is_return=True)
        params = params.strip()
        if params in ("void", ""):
            if params == "":
                raise HeaderError(f"{name}: `()` declares no prototype in C; write `(void)`")
            args = []
        else:
            args = [_param_type(p, f"{name} (parameter {i})") for i, p in enumerate(params.split(","))]
        out[name] = (res, args)
    return out


_NAME_OF = {C.c_void_p: "c_void_p", C.c_char_p: "c_char_p", C.c_int: "c_int", C.c_longlong: "c_longlong", C.c_float: "c_float",
            C.c_uint: "c_uint", C.c_size_t: "c_size_t", C.c_double: "c_double"}   # ctypes aliases equal widths (c_longlong is c_long)


def _n(t):
    return _NAME_OF.get(t) or getattr(t, "__name__", repr(t))


def compare(header, prototypes):
    """Every difference between the parsed header and a PROTOTYPES-like table, as (name, index, header type, python type):
    index -1 is the return type, None a name or a parameter count."""
    bad = []
    for name in sorted(set(header) | set(prototypes)):
        if name not in prototypes:
            bad.append((name, None, "declared", "no prototype"))
            continue
        if name not in header:
            bad.append((name, None, "not declared", "prototype"))
            continue
        (hres, hargs), (pres, pargs) = header[name], prototypes[name]
        if hres is not pres:
            bad.append((name, -1, _n(hres), _n(pres)))
        for i, (h, p) in enumerate(zip(hargs, pargs)):
            if h is not p:
                bad.append((name, i, _n(h), _n(p)))
        if len(hargs) != len(pargs):
            i = min(len(hargs), len(pargs))
            bad.append((name, i, _n(hargs[i]) if i < len(hargs) else "end of list", _n(pargs[i]) if i < len(pargs) else "end of list"))
    return bad


# ---- the registry -------------------------------------------------------------------------------------------------------------
# The census below runs once per header of ecm_amd._lib.TABLES.  The names are spelled out here because parametrize needs them
# before the package is imported; test_the_census_covers_every_table holds this list to the registry.
HEADERS = ("ecm_hip.h", "ecm_geometry.h", "ecm_rectify.h")
TABLE_NAME = {"ecm_hip.h": "PROTOTYPES", "ecm_geometry.h": "GEOMETRY_PROTOTYPES", "ecm_rectify.h": "RECTIFY_PROTOTYPES"}
ENTRIES_IN = {"ecm_geometry.h": "test_disp_reproject_cpu", "ecm_rectify.h": "test_rectify_cpu"}   # modules with an ENTRIES list
census = pytest.mark.parametrize("header", HEADERS)


def registry():
    import ecm_amd
    return ecm_amd._lib.TABLES


def prototypes(header="ecm_hip.h"):
    return registry()[header][0]


def header_prototypes(header="ecm_hip.h"):
    with open(os.path.join(INCLUDE, header)) as f:
        return parse_header(f.read())


def declared(header="ecm_hip.h"):
    """The set of names `header` declares, by a plain search of its text without comments: what a per-op test asks "is my entry
    declared" of, and the count that the census holds parse_header to."""
    with open(os.path.join(INCLUDE, header)) as f:
        return set(re.findall(rf"\b({registry()[header][1]}[a-z0-9_]+)\s*\(", _strip(f.read())))


@pytest.fixture(scope="module")
def lib_mod():
    import ecm_amd
    if not os.path.exists(ecm_amd._lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return ecm_amd._lib


# ---- the census: every header against its table --------------------------------------------------------------------------------

def test_the_census_covers_every_table():
    import ecm_amd
    assert tuple(registry()) == HEADERS and all(os.path.exists(os.path.join(INCLUDE, h)) for h in HEADERS)
    assert all(registry()[h][0] is getattr(ecm_amd._lib, TABLE_NAME[h]) for h in HEADERS)    # the dicts that tests mutate in place


@census
def test_every_declaration_parses_and_is_counted(header):
    table, prefix = registry()[header]
    parsed = header_prototypes(header)                                              # an unknown type raises, naming the declaration
    assert sorted(parsed) == sorted(declared(header)) == sorted(table)
    assert len(parsed) == len(declared(header)) == len(table) > 0
    assert all(n.startswith(prefix) for n in parsed)
    if header in ENTRIES_IN:
        assert sorted(parsed) == sorted(importlib.import_module(ENTRIES_IN[header]).ENTRIES)
    tables = [set(t) for t, _ in registry().values()]
    for i, a in enumerate(tables):                                                  # all the tables, pairwise disjoint
        for b in tables[i + 1:]:
            assert not a & b, sorted(a & b)


@census
def test_prototypes_match_header_type_by_type(header):
    table, parsed = prototypes(header), header_prototypes(header)
    bad = compare(parsed, table)
    assert not bad, "\n".join(f"{n}: {'return' if i == -1 else 'names' if i is None else f'parameter {i}'}: header {h}, _lib.py {p}"
                              for n, i, h, p in bad)
    compared = [n for n in parsed if table[n] == parsed[n]]                         # the equality the table is used by, row by row
    assert len(compared) == len(parsed) == len(table)


@census
def test_library_exports_every_row_and_load_types_it(header, lib_mod):
    table, prefix = registry()[header]
    lib = C.CDLL(lib_mod.LIB_PATH)
    assert [n for n in sorted(declared(header)) if not hasattr(lib, n)] == []
    assert lib_mod.missing_symbols() == []
    real = dict(table)
    try:                                                                            # missing_symbols() covers this table, in place
        table[prefix + "not_there"] = (C.c_int, [])
        assert lib_mod.missing_symbols() == [prefix + "not_there"]
    finally:
        table.clear()
        table.update(real)
    loaded = lib_mod.load()
    for name, (res, args) in table.items():                                         # load() typed them
        assert getattr(loaded, name).restype is res and list(getattr(loaded, name).argtypes) == args, name
    with pytest.raises(RuntimeError, match="does not export"):
        lib_mod.call(prefix + "not_there")


def test_parser_reads_the_forms_the_header_uses():
    got = parse_header("""
        /* int commented_out(int a); */
        #define ECM_X (-1)
        int         ecm_a(void);            /* trailing */
        const char* ecm_b(int code);
        long long ecm_c(int B, int C, long long HW);
        int ecm_d(const float* const* measures, long long* count, const unsigned char* v, const unsigned short* x,
                  const int* h, void* scratch, long long scratch_bytes,
                  float eps, void* stream);
        unsigned ecm_e(unsigned int n, size_t bytes, double x, const void *p, float);
    """)
    _I, _LL, _F, _P = C.c_int, C.c_longlong, C.c_float, C.c_void_p
    assert got == {
        "ecm_a": (_I, []),
        "ecm_b": (C.c_char_p, [_I]),
        "ecm_c": (_LL, [_I, _I, _LL]),
        "ecm_d": (_I, [_P, _P, _P, _P, _P, _P, _LL, _F, _P]),
        "ecm_e": (C.c_uint, [C.c_uint, C.c_size_t, C.c_double, _P, _F]),
    }


# ---- the comparer can fail: planted defects ----------------------------------------------------------------------------------

_I, _LL, _F, _P = C.c_int, C.c_longlong, C.c_float, C.c_void_p
PLANTED = [
    ("long long against _I",
     "int ecm_x(const float* c0, long long head_stride, float* disp, int B, void* stream);",
     {"ecm_x": (_I, [_P, _I, _P, _I, _P])},
     [("ecm_x", 1, "c_longlong", "c_int")]),
    ("float and int swapped between neighbours",
     "int ecm_x(const float* dl, int W, float threshold, float rel,\n          int mirrored, void* stream);",
     {"ecm_x": (_I, [_P, _I, _F, _I, _F, _P])},
     [("ecm_x", 3, "c_float", "c_int"), ("ecm_x", 4, "c_int", "c_float")]),
    ("missing trailing void* stream",
     "int ecm_x(const float* x, float* y, int n, void* stream);",
     {"ecm_x": (_I, [_P, _P, _I])},
     [("ecm_x", 3, "c_void_p", "end of list")]),
    ("extra trailing parameter",
     "int ecm_x(const float* x, float* y, int n, void* stream);",
     {"ecm_x": (_I, [_P, _P, _I, _P, _P])},
     [("ecm_x", 4, "end of list", "c_void_p")]),
    ("int return against _LL",
     "int ecm_x_max(void);",
     {"ecm_x_max": (_LL, [])},
     [("ecm_x_max", -1, "c_int", "c_longlong")]),
    ("long long return against _I",
     "long long ecm_x_scratch_bytes(int B, long long n);",
     {"ecm_x_scratch_bytes": (_I, [_I, _LL])},
     [("ecm_x_scratch_bytes", -1, "c_longlong", "c_int")]),
    ("c_int standing for unsigned",
     "int ecm_x(unsigned n, void* stream);",
     {"ecm_x": (_I, [_I, _P])},
     [("ecm_x", 0, "c_uint", "c_int")]),
]


@pytest.mark.parametrize("header,table,want", [p[1:] for p in PLANTED], ids=[p[0] for p in PLANTED])
def test_comparer_reports_planted_defect(header, table, want):
    assert compare(parse_header(header), table) == want


@pytest.mark.parametrize("header,named", [
    ("int ecm_x(const float* x, hipStream_t stream);", "ecm_x (parameter 1)"),
    ("int ecm_x(int64_t n, void* stream);", "ecm_x (parameter 0)"),
    ("int ecm_x(int n, int (*cb)(int), void* stream);", "ecm_x"),
    ("float* ecm_x(int n);", "ecm_x (return)"),
    ("int ecm_x(const struct ecm_desc* d);", "ecm_x (parameter 0)"),
    ("int ecm_x();", "ecm_x"),
], ids=["typedef", "int64_t", "function pointer", "pointer return", "struct pointee", "no prototype"])
def test_unknown_type_fails_and_names_the_declaration(header, named):
    with pytest.raises(HeaderError) as e:
        parse_header(header)
    assert named in str(e.value)


def test_clean_synthetic_header_compares_equal():
    h = "long long ecm_q(int B, long long S);\nint ecm_r(const float* x, float eps, long long S, void* stream);"
    assert compare(parse_header(h), {"ecm_q": (_LL, [_I, _LL]), "ecm_r": (_I, [_P, _F, _LL, _P])}) == []
    assert compare(parse_header(h), {"ecm_q": (_LL, [_I, _LL])}) == [("ecm_r", None, "declared", "no prototype")]


# ---- the call sites ----------------------------------------------------------------------------------------------------------

# Entry points that no Python source of the package names: each with the reason it stays in the ABI and the caller that keeps
# it honest.  tests/test_hip_abi_calls.py closes on the same table: recorded calls + ABI_ONLY == PROTOTYPES.
ABI_ONLY = {
    "ecm_abi_version": ("build information for hosts of the C ABI; the package checks symbols, not the number",
                        "tests/test_abi.py::test_version_and_error_strings, tests/c_host/chain_host.cpp"),
    "ecm_error_string": ("reached only as an attribute of the loaded library on the error path (lib.ecm_error_string(rc) in "
                         "_lib.call and ops.check_async_errors), never by name through _lib.call / _lib.query",
                         "tests/test_abi.py::test_version_and_error_strings, tests/c_host/costvol_host.cpp"),
    "ecm_gn3d_apply": ("the fp32 -> fp32 two-stage GroupNorm apply: the library's own fallback inside ecm_gn3d_fwd, exported for "
                       "hosts that keep the statistics", "tests/test_hip_abi_calls.py::test_gn3d_apply_from_a_host"),
    "ecm_gn3d_poll_ms": ("the wait bound of the cluster kernels, a diagnostic control", "tests/test_gn_cluster.py"),
}


def package_entry_names(pattern=r"ecm_[a-z0-9_]+", table_name="PROTOTYPES"):
    """{name: ["file:line", ...]} of every entry point the package's Python sources name: a whole string literal matching
    `pattern` (what _lib.call, _lib.query, _call_scratch, _gn_launch and the tables they are fed from receive).  The sources are
    walked as syntax trees, so comments do not count; docstrings, pieces of f-strings (labels of error messages) and the
    assignment of `table_name` in _lib.py, the table itself, are left out."""
    found = {}
    for fn in sorted(os.listdir(PACKAGE)):
        if not fn.endswith(".py"):
            continue
        with open(os.path.join(PACKAGE, fn)) as f:
            tree = ast.parse(f.read(), fn)
        skip = set()
        for node in ast.walk(tree):
            if fn == "_lib.py" and isinstance(node, (ast.Assign, ast.AnnAssign)):
                tgt = node.targets[0] if isinstance(node, ast.Assign) else node.target
                if isinstance(tgt, ast.Name) and tgt.id == table_name:
                    skip.update(id(n) for n in ast.walk(node))
            if isinstance(node, ast.JoinedStr):
                skip.update(id(n) for n in ast.walk(node))
            if isinstance(node, (ast.Module, ast.ClassDef, ast.FunctionDef, ast.AsyncFunctionDef)) and node.body \
                    and isinstance(node.body[0], ast.Expr) and isinstance(node.body[0].value, ast.Constant):
                skip.add(id(node.body[0].value))
        for node in ast.walk(tree):
            if id(node) in skip:
                continue
            if isinstance(node, ast.Constant) and isinstance(node.value, str) and re.fullmatch(pattern, node.value):
                found.setdefault(node.value, []).append(f"{fn}:{node.lineno}")
    return found


def entry_names_of(header):
    return package_entry_names(registry()[header][1] + "[a-z0-9_]+", TABLE_NAME[header])


@census
def test_every_name_the_package_passes_is_a_prototype(header):
    found, table = entry_names_of(header), prototypes(header)
    assert len(found) >= (100 if header == "ecm_hip.h" else len(table)), len(found)  # the walk sees the call sites at all
    unknown = {n: at for n, at in found.items() if n not in table}
    assert not unknown, f"named in the package but absent from {TABLE_NAME[header]}: {unknown}"
    if header != "ecm_hip.h":                                                       # the small tables: ops.py alone names them
        assert all(a.startswith("ops.py:") for at in found.values() for a in at), found


def test_no_entry_name_is_built_from_pieces():
    """A name assembled at run time (name + "_scratch_bytes", an f-string) is invisible to the walk above and to grep: the callers
    of the library take their names as whole literals, directly or through a variable."""
    callers = {"call", "query", "_call_scratch", "_gn_call", "_gn_launch"}
    built = []
    for fn in sorted(os.listdir(PACKAGE)):
        if not fn.endswith(".py"):
            continue
        with open(os.path.join(PACKAGE, fn)) as f:
            tree = ast.parse(f.read(), fn)
        for node in ast.walk(tree):
            if isinstance(node, ast.Call) and getattr(node.func, "attr", getattr(node.func, "id", None)) in callers:
                for a in node.args:
                    if isinstance(a, (ast.BinOp, ast.JoinedStr)) and \
                            any(isinstance(c, ast.Constant) and isinstance(c.value, str) for c in ast.walk(a)):
                        built.append(f"{fn}:{a.lineno}")
    assert not built, f"entry-point names built from pieces at {built}"


@census
def test_every_prototype_is_reached_or_accounted_for(header):
    """Every row is named by the package or, in ecm_hip.h alone, accounted for in ABI_ONLY: the other tables have no such rows."""
    found, table = set(entry_names_of(header)), set(prototypes(header))
    abi_only = set(ABI_ONLY) if header == "ecm_hip.h" else set()
    stale = sorted(abi_only & found)
    assert not stale, f"in ABI_ONLY although the package calls them: {stale}"
    assert not abi_only - table, sorted(abi_only - table)
    orphans = sorted(table - found - abi_only)
    assert not orphans, f"in {TABLE_NAME[header]}, called by nothing in the package and not in ABI_ONLY: {orphans}"
    assert all(reason and caller for reason, caller in ABI_ONLY.values())


def test_abi_only_callers_exist():
    """Each ABI_ONLY row names the file(s) that call the entry; the name must really appear there."""
    for name, (_, callers) in ABI_ONLY.items():
        for c in callers.split(","):
            path = os.path.join(ROOT, c.strip().split("::")[0])
            with open(path) as f:
                assert name in f.read(), f"{name}: not called in {c.strip()}"
