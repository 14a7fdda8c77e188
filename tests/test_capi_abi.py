"""htk_amd/abi.py: the ctypes prototypes of the C ABI come from include/htk_amd.h, all of them, and the struct mirrors of
htk_amd/capi.py have the C structs' layout.  No GPU."""
import ctypes as C
import os
import re
import subprocess

import pytest

from htk_amd import abi
from test_capi_symbols import declared_functions

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
c_int, c_float, c_double, c_void_p, c_char_p = C.c_int, C.c_float, C.c_double, C.c_void_p, C.c_char_p


@pytest.fixture(scope="module")
def table(native):
    return abi.prototypes(native.STRUCTS)


def test_every_declared_function_has_a_prototype(native, table):
    assert set(table) == set(declared_functions())
    L = native.lib()
    scalars = set(abi.SCALARS.values())
    for name, (res, args) in table.items():
        assert hasattr(L, name), name
        f = getattr(L, name)
        assert f.argtypes is not None and list(f.argtypes) == args and f.restype is res, name
        # nothing fell back to a default: every type is one the mapping names
        for t in args:
            assert t in scalars or t in (c_void_p, c_char_p), (name, t)
        assert res is None or res in scalars or res in (c_void_p, c_char_p, C.POINTER(c_float)) or issubclass(res._type_, C.Structure), (name, res)
    # and the library exports nothing of the ABI that the table misses
    syms = subprocess.run(["nm", "-D", "--defined-only", native.LIBPATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (htkamd_\w+)$", syms, flags=re.M))
    assert exported, "nm shows no htkamd_ symbols"
    for name in exported & set(table):
        assert getattr(L, name).argtypes is not None, name


def test_known_answers(native, table):
    assert table["htkamd_dev_malloc"] == (c_int, [c_void_p, C.c_size_t])
    assert table["htkamd_trans_add"] == (c_int, [c_void_p, c_double, c_double, c_char_p, c_float, c_char_p, c_float, c_char_p, c_float])
    assert table["htkamd_labels_start"][0] is C.c_longlong
    assert table["htkamd_scp_start"][0] is C.c_long
    assert table["htkamd_results_last_kernel_ms"][0] is c_double
    assert table["htkamd_model_destroy"] == (None, [c_void_p])
    assert table["htkamd_mmf_desc"][0] is C.POINTER(native.ModelDesc)
    assert table["htkamd_net_get"][0] is C.POINTER(native.NetDesc)
    assert table["htkamd_mmf_var_floor"][0] is C.POINTER(c_float)
    assert table["htkamd_mlf_find"] == (c_void_p, [c_void_p, c_char_p])
    assert table["htkamd_name_question_answers"][1][0] is c_void_p                       # const char *const *names
    assert table["htkamd_fb_mix_counts"] == (c_int, [c_void_p, c_void_p])                  # long long out[2]
    assert table["htkamd_model_get_prepared"] == (c_int, [c_void_p] * 5)                   # two lines, /*[n]*/ inside the list
    assert table["htkamd_version"] == (c_int, [])
    assert table["htkamd_regtree_probe"] == (c_int, [c_void_p] * 5 + [c_int, c_int, c_void_p, c_void_p, c_int] + [c_void_p] * 4)      # three lines
    # the decoder set's entries, as its tests knew them when lib() declared them by hand
    assert table["htkamd_decoder_set_run"][1][4] is c_void_p and len(table["htkamd_decoder_set_run"][1]) == 9
    for s in ("htkamd_decoder_set_create", "htkamd_decoder_set_destroy", "htkamd_decoder_set_run", "htkamd_decoder_set_last_tied",
              "htkamd_decoder_set_run_lattice", "htkamd_decoder_set_run_lattice_align"):
        assert getattr(native.lib(), s).argtypes, s
    for s in ("htkamd_decoder_set_run_lattice", "htkamd_decoder_set_run_lattice_align"):
        assert getattr(native.lib(), s).restype is c_int, s
    assert len(table["htkamd_decoder_set_run_lattice"][1]) == 12 and len(table["htkamd_decoder_set_run_lattice_align"][1]) == 15
    assert table["htkamd_decoder_set_run_lattice"][1][3] is c_float and table["htkamd_decoder_set_run_lattice_align"][1][4] is c_int


def test_an_unknown_type_is_an_error(native):
    for bad in ("int htkamd_x(uint64_t n);", "short htkamd_x(void);", "int *htkamd_x(void);", "int htkamd_x(int (*f)(int));",
                "typedef struct { int a; } htkamd_new;\nint htkamd_x(const htkamd_new *p);", "int htkamd_x(void) { return 0; }"):
        with pytest.raises(ValueError):
            abi.prototypes(native.STRUCTS, bad)
    assert abi.prototypes(native.STRUCTS, "#define A \\\n  int\n/* int htkamd_y(void); */ void htkamd_x(const unsigned char *a /*[n]*/,\n short *b);") \
        == {"htkamd_x": (None, [c_void_p, c_void_p])}


def test_struct_mirrors_have_the_c_layout(native, tmp_path):
    """sizeof and every field's offsetof, by the C compiler, for all structs of the header."""
    header = open(abi.HEADER).read()
    mirrors = [v for v in vars(native).values() if isinstance(v, type) and issubclass(v, C.Structure) and v is not C.Structure]
    assert sorted(abi.struct_names(header)) == sorted(native.STRUCTS) and len(native.STRUCTS) == len(set(native.STRUCTS.values()))
    assert set(mirrors) == set(native.STRUCTS.values())
    lines, want = [], []
    for cname, m in sorted(native.STRUCTS.items()):
        lines.append('printf("%%zu\\n", sizeof(%s));' % cname); want.append(C.sizeof(m))
        for f, _ in m._fields_:
            lines.append('printf("%%zu\\n", offsetof(%s, %s));' % (cname, f)); want.append(getattr(m, f).offset)
        body = re.search(r"typedef\s+struct\s*\{([^{}]*)\}\s*%s\s*;" % cname, re.sub(r"/\*.*?\*/", " ", header, flags=re.S)).group(1)
        nC = sum(d.count(",") + 1 for d in body.split(";") if d.strip())
        assert nC == len(m._fields_), "%s: %d fields in the header, %d in the mirror" % (cname, nC, len(m._fields_))
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "htk_amd.h"\nint main(void) {\n%s\nreturn 0; }\n' % "\n".join(lines))
    subprocess.check_call(["gcc", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "layout")])
    got = [int(x) for x in subprocess.check_output([str(tmp_path / "layout")], text=True).split()]
    assert got == want


def test_bare_python_values_travel_whole(native):
    """A handle as a plain int and a bare index: what ctypes cut to a C int before the prototypes were declared."""
    L = native.lib()
    h = c_void_p()
    native.check(L.htkamd_labels_read(os.path.join(ROOT, "tests", "golden", "demo", "labels", "tr1.lab").encode(), C.byref(h)), "labels_read")
    try:
        assert isinstance(h.value, int)
        assert L.htkamd_labels_count(h.value) > 5
        assert [L.htkamd_labels_name(h.value, i) for i in range(5)] == [b"S", b"C", b"V", b"C", b"V"]
        assert [L.htkamd_labels_start(h.value, i) for i in range(3)] == [0, 1410000, 2591250]
        assert L.htkamd_labels_end(h.value, 4) == 4535000
        with pytest.raises(C.ArgumentError):
            L.htkamd_labels_name(h.value, 1.0)
    finally:
        L.htkamd_labels_free(h)
