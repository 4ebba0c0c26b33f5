"""The rasterizer's argument structs (include/gsr.h gsr_scene, gsr_view, gsr_forward_args, gsr_backward_args) and
their ctypes mirrors in gaussian_splatting_amd/_lib.py, held together without a GPU: a C program that includes
gsr.h prints sizeof and every field's offsetof and size, which must equal the mirrors' name by name; and the two
entry points' argument checks that return before any HIP call.
"""
import ctypes
import re
import subprocess

import pytest

from gaussian_splatting_amd import _lib, build

STRUCTS = {"gsr_scene": _lib.Scene, "gsr_view": _lib.View, "gsr_forward_args": _lib.ForwardArgs,
           "gsr_backward_args": _lib.BackwardArgs}


def _header_fields(text):
    """{struct: [(field, nested struct name or None)]} of the typedef'd structs in the header, comments removed."""
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    out = {}
    for body, name in re.findall(r"typedef\s+struct\s+\w+\s*\{(.*?)\}\s*(\w+)\s*;", text, flags=re.S):
        fields = []
        for decl in filter(None, (d.strip() for d in body.split(";"))):
            first, *more = decl.split(",")
            *type_words, ident = first.replace("*", " * ").split()
            nested = type_words[0] if type_words[0] in STRUCTS else None
            for ident in [ident] + [m.replace("*", " ").split()[-1] for m in more]:
                assert re.fullmatch(r"[A-Za-z_]\w*", ident), (name, decl)
                fields.append((ident, nested))
        out[name] = fields
    return out


def _flatten_header(fields, name):
    for ident, nested in fields[name]:
        yield ident
        if nested:
            for sub in _flatten_header(fields, nested):
                yield f"{ident}.{sub}"


def _flatten_ctypes(cls, prefix="", base=0):
    for ident, typ in cls._fields_:
        d = getattr(cls, ident)
        yield prefix + ident, (base + d.offset, d.size)
        if issubclass(typ, ctypes.Structure):
            yield from _flatten_ctypes(typ, prefix + ident + ".", base + d.offset)


@pytest.fixture(scope="module")
def c_layout(tmp_path_factory):
    """{struct: {"sizeof": n, field path: (offset, size)}} as the C compiler lays gsr.h out."""
    fields = _header_fields(open(_lib.HEADER_PATH).read())
    assert set(STRUCTS) <= set(fields), sorted(fields)
    lines = ["#include <stddef.h>", "#include <stdio.h>", '#include "gsr.h"', "int main(void) {"]
    for s in STRUCTS:
        lines.append(f'    printf("{s} sizeof %zu 0\\n", sizeof({s}));')
        for path in _flatten_header(fields, s):
            lines.append(f'    printf("{s} {path} %zu %zu\\n", offsetof({s}, {path}), sizeof((({s}*)0)->{path}));')
    lines += ["    return 0;", "}", ""]
    d = tmp_path_factory.mktemp("abi_layout")
    src, exe = d / "layout.c", d / "layout"
    src.write_text("\n".join(lines))
    r = subprocess.run([build.HIPCC, "-x", "c", "-std=c11", "-Wall", "-Werror", "-I", _lib.INCLUDE_DIR, str(src), "-o",
                        str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout
    layout = {s: {} for s in STRUCTS}
    for line in out.splitlines():
        s, path, a, b = line.split()
        layout[s][path] = int(a) if path == "sizeof" else (int(a), int(b))
    return layout


@pytest.mark.parametrize("struct", sorted(STRUCTS))
def test_ctypes_mirror_has_the_headers_layout(c_layout, struct):
    cls = STRUCTS[struct]
    want = dict(c_layout[struct])
    assert ctypes.sizeof(cls) == want.pop("sizeof")
    got = dict(_flatten_ctypes(cls))
    assert set(got) == set(want), (sorted(set(got) - set(want)), sorted(set(want) - set(got)))
    for name in want:
        assert got[name] == want[name], (name, got[name], want[name])
    # the order too: a mirror listing the header's fields in the header's order
    assert list(got) == list(want)


def test_args_carry_their_own_size():
    assert _lib.ForwardArgs().struct_size == ctypes.sizeof(_lib.ForwardArgs)
    assert _lib.BackwardArgs(R=3).struct_size == ctypes.sizeof(_lib.BackwardArgs)
    assert _lib.ForwardArgs._fields_[0][0] == _lib.BackwardArgs._fields_[0][0] == "struct_size"


@pytest.fixture(scope="module")
def lib():
    build.build(verbose=False)
    return _lib.load()


def test_wrong_struct_size_is_refused_and_both_sizes_named(lib):
    a = _lib.BackwardArgs()
    a.struct_size = ctypes.sizeof(a) - 8
    assert lib.gsr_rasterize_backward(ctypes.byref(a)) == 1  # GSR_ERR_ARGUMENT
    msg = lib.gsr_last_error().decode()
    assert str(ctypes.sizeof(a)) in msg and str(ctypes.sizeof(a) - 8) in msg, msg
    f = _lib.ForwardArgs()
    f.struct_size = 0
    assert lib.gsr_rasterize_forward(ctypes.byref(f)) == 1
    assert str(ctypes.sizeof(f)) in lib.gsr_last_error().decode()


def test_negative_point_count_is_invalid_sizes(lib):
    view = _lib.View(width=16, height=16)
    f = _lib.ForwardArgs(scene=_lib.Scene(P=-1), view=view)
    assert lib.gsr_rasterize_forward(ctypes.byref(f)) == 1
    assert "invalid sizes" in lib.gsr_last_error().decode()
    b = _lib.BackwardArgs(scene=_lib.Scene(P=-1), view=view)
    assert lib.gsr_rasterize_backward(ctypes.byref(b)) == 1
    assert "invalid sizes" in lib.gsr_last_error().decode()


def test_no_gaussians_is_ok_and_launches_nothing(lib):
    view = _lib.View(width=16, height=16)
    f = _lib.ForwardArgs(scene=_lib.Scene(P=0), view=view, num_rendered=7, binning_capacity=7)
    assert lib.gsr_rasterize_forward(ctypes.byref(f)) == 0, lib.gsr_last_error()
    assert f.num_rendered == 0 and f.binning_capacity == 0
    b = _lib.BackwardArgs(scene=_lib.Scene(P=0), view=view, R=f.num_rendered)
    assert lib.gsr_rasterize_backward(ctypes.byref(b)) == 0, lib.gsr_last_error()
    assert lib.gsr_last_error() == b""
