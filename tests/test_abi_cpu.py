"""CPU: the ctypes binding (<pkg>/_abi.py) against include/qtcnn.h -- the signature table against every prototype, the
struct mirrors against the C compiler's layout, 64-bit values across the boundary, bind() itself, and no argtypes /
restype / ctypes.Structure anywhere else.  Host code only: no entry point called here touches a device."""
import ast
import ctypes
import glob
import os
import re
import subprocess

import pytest

from _util import PKG, ROOT, pkg

HEADER = os.path.join(ROOT, "include", "qtcnn.h")
LIB_PATH = os.path.join(ROOT, PKG, "libqtcnn_hip.so")
SCALARS = {"int": ctypes.c_int, "long long": ctypes.c_longlong, "unsigned long long": ctypes.c_ulonglong,
           "size_t": ctypes.c_size_t, "float": ctypes.c_float, "double": ctypes.c_double}
# the one mirror whose field names are not the header's: qt_conv_io.bwd_bn[2] is flattened
ALIASES = {"ConvIO": {f"bn{i}_{m}": f"bwd_bn[{i}].{m}" for i in (0, 1) for m in ("y", "mean", "invstd", "partial")}}


def _built():
    if not os.path.exists(LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return LIB_PATH


def _header():
    src = open(HEADER).read()
    return re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", src, flags=re.S))


def _ctype(c, is_return=False):
    """The mapping rule of _abi.py, restated: scalars directly, char* is c_char_p, void return None, other pointers c_void_p."""
    c = " ".join(c.replace("*", " * ").split())
    if "*" in c:
        return ctypes.c_char_p if c.replace("const ", "") == "char *" else ctypes.c_void_p
    c = c.replace("const ", "")
    return None if (c == "void" and is_return) else SCALARS[c]


def _prototypes():
    out = {}
    prototype = r"(?m)^\s*((?:const\s+)?[A-Za-z_][\w ]*?[\s*]+)(qt_\w+)\s*\(([^)]*)\)\s*;"   # ret qt_name(args);
    for ret, name, args in re.findall(prototype, _header()):
        args = " ".join(args.split())
        params = [] if args == "void" else [re.match(r"(.*?)\w+$", a.strip()).group(1) for a in args.split(",")]
        assert name not in out, name
        out[name] = (_ctype(ret, True), [_ctype(p) for p in params])
    return out


def _struct_bodies():
    return dict(re.findall(r"typedef struct (qt_\w+) \{(.*?)\n\} \1;", _header(), flags=re.S))


def _declarators(body):
    """Number of member declarators of a struct body; an anonymous `struct { ... } name[N]` counts N times its members."""
    n = 0
    for inner, count in re.findall(r"struct \{(.*?)\}\s*\w+\[(\d+)\]\s*;", body, flags=re.S):
        n += int(count) * _declarators(inner)
    body = re.sub(r"struct \{.*?\}\s*\w+\[\d+\]\s*;", "", body, flags=re.S)
    return n + sum(len(decl.split(",")) for decl in body.split(";") if decl.strip())


def _mirrors():
    """{C struct name: mirror class}, from the `# qt_xxx` comment each class of _abi.py carries."""
    abi = pkg("_abi")
    src = open(os.path.join(ROOT, PKG, "_abi.py")).read()
    named = dict(re.findall(r"(?m)^class (\w+)\(ctypes\.Structure\):\s*#\s*(qt_\w+)\s*$", src))
    classes = [n.name for n in ast.parse(src).body if isinstance(n, ast.ClassDef) and n.bases
               and ast.unparse(n.bases[0]).endswith("Structure")]
    assert sorted(classes) == sorted(named), "every struct mirror carries its `# qt_xxx` comment"
    return {c_name: getattr(abi, py_name) for py_name, c_name in named.items()}


def test_table_equals_header():
    abi = pkg("_abi")
    protos = _prototypes()
    assert len(protos) == 192
    assert set(abi.SIGNATURES) == set(protos)
    for name, (ret, params) in protos.items():
        restype, argtypes = abi.SIGNATURES[name]
        assert restype is ret, (name, "return", restype, ret)
        assert len(argtypes) == len(params), (name, "arity", len(argtypes), len(params))
        for i, (got, want) in enumerate(zip(argtypes, params)):
            assert got is want, (name, "parameter", i, got, want)
    lib = ctypes.CDLL(_built())
    missing = [name for name in sorted(protos) if not hasattr(lib, name)]
    assert not missing, missing


def test_struct_layouts_equal_the_c_compilers(tmp_path):
    mirrors, bodies = _mirrors(), _struct_bodies()
    assert len(bodies) == 27 and set(mirrors) == set(bodies)
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "qtcnn.h"', "int main(void) {"]
    for c_name, cls in mirrors.items():
        alias = ALIASES.get(cls.__name__, {})
        lines.append(f'  printf("{c_name} sizeof %zu\\n", sizeof({c_name}));')
        for field, _ in cls._fields_:
            lines.append(f'  printf("{c_name} {field} %zu\\n", offsetof({c_name}, {alias.get(field, field)}));')
    lines += ["  return 0;", "}"]
    source, exe = tmp_path / "layout.c", tmp_path / "layout"
    source.write_text("\n".join(lines) + "\n")
    subprocess.run(["cc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(source), "-o", str(exe)], check=True)
    printed = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n")
    c_layout = {tuple(line.split()[:2]): int(line.split()[2]) for line in printed if line}
    for c_name, cls in mirrors.items():
        assert ctypes.sizeof(cls) == c_layout[c_name, "sizeof"], (c_name, "sizeof")
        for field, _ in cls._fields_:
            assert getattr(cls, field).offset == c_layout[c_name, field], (c_name, field)
        # sizeof alone can hide a missing trailing int behind alignment padding
        assert len(cls._fields_) == _declarators(bodies[c_name]), (c_name, "number of fields")


def test_wide_values_cross_the_boundary_whole():
    _built()
    L = pkg("_lib").lib()
    # elementwise.hip: min(ceil(rows / 128), 1024) parts x max(cols, 1) columns x 4 bytes
    ws = L.qt_col_sum_workspace_bytes
    assert ws(2**32 + 128, 1) == ws(2**40, 1) == 4096
    assert ws(128, 1) == 4                        # what `rows` cut to 32 bits would give
    assert ws(2**40, 2**30) == 2**42              # 1024 * 2^30 * 4: a size_t return cut to 32 bits would be 0
    assert ws(2**40, 2**30) >= 2**32 and ws(2**40, 2**30) % 2**32 == 0
    # video3d.hip: min(max(ceil(M / 256), 1), 1024) rows
    rows = L.qt_bn_stats_rows
    assert rows(2**32 + 256, 8) == rows(2**40, 8) == 1024
    assert rows(256, 8) == 1


def test_bind_is_idempotent_and_types_any_handle():
    abi = pkg("_abi")
    first = ctypes.CDLL(_built())
    assert first.qt_col_sum_workspace_bytes.argtypes is None
    assert abi.bind(first) is first
    typed = {name: (getattr(first, name).restype, getattr(first, name).argtypes) for name in abi.SIGNATURES}
    for name, (restype, argtypes) in abi.SIGNATURES.items():
        assert typed[name][0] is restype and list(typed[name][1]) == list(argtypes), name
    assert abi.bind(first) is first               # the second bind() leaves every function as it is
    for name in abi.SIGNATURES:
        assert getattr(first, name).argtypes is typed[name][1], name
    second = abi.bind(ctypes.CDLL(LIB_PATH))
    assert second is not first
    assert second.qt_col_sum_workspace_bytes.restype is ctypes.c_size_t
    assert list(second.qt_bn_stats_rows.argtypes) == [ctypes.c_longlong, ctypes.c_int]
    stale = dict(abi.SIGNATURES, qt_no_such_entry_point=(ctypes.c_int, []))
    with pytest.raises(abi.QtError, match="qt_no_such_entry_point.*stale"):
        abi.bind(ctypes.CDLL(LIB_PATH), stale)


def test_no_signature_or_struct_outside_the_abi_module():
    files = [p for p in glob.glob(os.path.join(ROOT, PKG, "**", "*.py"), recursive=True)
             if os.path.relpath(p, os.path.join(ROOT, PKG)) != "_abi.py"]
    files += glob.glob(os.path.join(ROOT, "tests", "*.py")) + glob.glob(os.path.join(ROOT, "scripts", "*.py"))
    assert len(files) > 150
    strays = []
    for path in files:
        for node in ast.walk(ast.parse(open(path).read())):
            targets = []
            if isinstance(node, ast.Assign):
                targets = node.targets
            elif isinstance(node, (ast.AugAssign, ast.AnnAssign)):
                targets = [node.target]
            for t in targets:
                for leaf in ast.walk(t):
                    if isinstance(leaf, ast.Attribute) and leaf.attr in ("argtypes", "restype"):
                        strays.append((os.path.relpath(path, ROOT), node.lineno, leaf.attr))
            if isinstance(node, ast.ClassDef) and any(ast.unparse(b).split(".")[-1] in ("Structure", "Union") for b in node.bases):
                strays.append((os.path.relpath(path, ROOT), node.lineno, node.name))
    assert not strays, strays
