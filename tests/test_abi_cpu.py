"""The ctypes binding is derived from include/sepr.h (sepreformer_amd/abi.py).  Three things hold the line, none needs a device:
the derived binding equals, entry for entry, the hand-written one of the parent commit (tests/golden/abi_binding.json, recorded by
tests/golden/make_abi_golden.py); the struct layouts and constants equal what the host C compiler makes of the header; and the reader
reads - an altered header changes exactly what was altered, and whatever lies outside its subset raises with the line."""
import ctypes as C
import importlib.util
import json
import os
import shutil
import subprocess
import sys

import pytest

from sepreformer_amd import abi
from sepreformer_amd import lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(ROOT, "include", "sepr.h")) as _f:
    HDR = _f.read()
H = abi.parse(HDR)
_spec = importlib.util.spec_from_file_location("make_abi_golden", os.path.join(ROOT, "tests", "golden", "make_abi_golden.py"))
G = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(G)


def derive(text):
    """SIGNATURES of an altered header, with lib.py's own struct classes and host-array table."""
    return abi.signatures(abi.parse(text), L._CLASSES, L._HOST_ARRAYS)


def test_derived_binding_equals_the_parents_record():
    with open(os.path.join(ROOT, "tests", "golden", "abi_binding.json")) as f:
        want = json.load(f)
    got = json.loads(json.dumps(G.describe(L)))
    assert len(want["entries"]) == 105 and len(want["structs"]) == 29 and len(want["constants"]) == 47
    for section in want:
        assert set(got[section]) == set(want[section]), (section, set(got[section]) ^ set(want[section]))
        wrong = {k: (want[section][k], got[section][k]) for k in want[section] if got[section][k] != want[section][k]}
        assert not wrong, (section, wrong)
    assert got == want
    assert set(L.SIGNATURES) == set(H.protos) and set(L._STRUCTS) == set(H.structs)


def test_header_through_the_host_compiler(tmp_path):
    """sizeof and every offsetof of every struct, and the value of every enum member and define, as cc sees the header."""
    cc = shutil.which("cc")
    if cc is None:
        pytest.skip("no host C compiler (cc) on the path")
    out = ['#include <stdio.h>', '#include <stddef.h>', '#include "sepr.h"', 'int main(void) {']
    for s, fields in H.structs.items():
        out.append(f'  printf("{s} sizeof %zu\\n", sizeof({s}));')
        out += [f'  printf("{s} {f} %zu\\n", offsetof({s}, {f}));' for _, f in fields]
    out += [f'  printf("value {k} %lld\\n", (long long)({k}));' for k in list(H.enums) + list(H.defines)]
    out += ['  printf("sizes %zu %zu %zu\\n", sizeof(sepr_stream_t), sizeof(sepr_u64), sizeof(size_t));', '  return 0;', '}']
    (tmp_path / "probe.c").write_text("\n".join(out) + "\n")
    subprocess.run([cc, "-I", os.path.join(ROOT, "include"), "-o", str(tmp_path / "probe"), str(tmp_path / "probe.c")], check=True)
    rows = [r.split() for r in subprocess.run([str(tmp_path / "probe")], check=True, capture_output=True, text=True).stdout.splitlines()]
    got = {(a, b): int(v) for a, b, v in rows[:-1]}
    want = {("value", k): v for k, v in {**H.enums, **H.defines}.items()}
    assert len(H.structs) == 29 and len(H.enums) == 53 and len(H.defines) == 5
    for s, fields in H.structs.items():
        cls = getattr(L, L._STRUCTS[s])
        assert [f for f, _ in cls._fields_] == [f for _, f in fields]
        want[(s, "sizeof")] = C.sizeof(cls)
        want.update({(s, f): getattr(cls, f).offset for _, f in fields})
    assert got == want, {k: (got.get(k), want.get(k)) for k in set(got) | set(want) if got.get(k) != want.get(k)}
    assert rows[-1] == ["sizes", str(C.sizeof(C.c_void_p)), str(C.sizeof(L._u64)), str(C.sizeof(L._sz))]
    # lib.py's public constants are those values
    for k, v in H.enums.items():
        if k.startswith(("SEPR_OP_", "SEPR_SITE_", "SEPR_TOP_", "SEPR_KNOB_")) and not k.endswith("_COUNT"):
            assert getattr(L, k[5:]) == got[("value", k)] == v
    assert {"SEPR_LEDGER_" + k.upper(): v for k, v in L.LEDGER_SLOTS.items()} == \
        {k: got[("value", k)] for k in H.enums if k.startswith("SEPR_LEDGER_") and k != "SEPR_LEDGER_MAX_PARTS"}
    assert L.LEDGER_MAX_PARTS == got[("value", "SEPR_LEDGER_MAX_PARTS")] and L.ABI_VERSION == got[("value", "SEPR_VERSION")]
    assert [L.SEPR_OK, L.SEPR_EINVAL, L.SEPR_EWORKSPACE, L.SEPR_EHIP] == [got[("value", k)] for k in ("SEPR_OK", "SEPR_EINVAL", "SEPR_EWORKSPACE", "SEPR_EHIP")]


def test_reader_forms():
    """Both kinds of comment (inside a declarator list too), several declarators, one-line structs, nested struct members, (void),
    a negative define, enum values set and implied."""
    h = abi.parse('''#define OUTSIDE 1
        extern "C" {
        #define A 7 /* a comment that
                       runs on */
        #define B (-2)   // to the end of the line
        typedef void* handle_t;
        typedef struct { const float* w /* [K] */; int n; } inner;
        typedef struct {
          inner a, /* first */ b,
                c;   // three of them
          float* const* p; unsigned long long q;
        } outer;
        enum { X = 3, Y, Z = -1, W, };
        const char* name(void);
        long long f(const outer* o, handle_t s /* the stream */, const int* const* t, double d);
        }''')
    assert h.defines == {"A": 7, "B": -2} and h.enums == {"X": 3, "Y": 4, "Z": -1, "W": 0} and h.typedefs == {"handle_t": "void*"}
    assert h.structs == {"inner": [("const float*", "w"), ("int", "n")],
                         "outer": [("inner", "a"), ("inner", "b"), ("inner", "c"), ("float* const*", "p"), ("unsigned long long", "q")]}
    assert h.protos == {"name": ("const char*", []),
                        "f": ("long long", [("const outer*", "o"), ("handle_t", "s"), ("const int* const*", "t"), ("double", "d")])}
    cls = abi.struct_classes(h, {"inner": "Inner", "outer": "Outer"})
    assert cls["outer"]._fields_ == [("a", cls["inner"]), ("b", cls["inner"]), ("c", cls["inner"]), ("p", C.c_void_p), ("q", C.c_ulonglong)]
    assert abi.signatures(h, cls, {"f": "t"}) == {"name": (C.c_char_p, []), "f": (C.c_longlong, [C.POINTER(cls["outer"]), C.c_void_p, C.POINTER(C.c_void_p), C.c_double])}
    assert abi.signatures(h, cls, {})["f"][1][2] is C.c_void_p


def test_an_altered_header_changes_exactly_what_was_altered():
    base = derive(HDR)
    assert base == L.SIGNATURES
    # long long total16 -> int total16, in one entry
    at = HDR.index("int sepr_dynmix_fwd(")
    got = derive(HDR[:at] + HDR[at:].replace("long long total16", "int total16", 1))
    i = [p for _, p in H.protos["sepr_dynmix_fwd"][1]].index("total16")
    assert base["sepr_dynmix_fwd"][1][i] is L._ll and got["sepr_dynmix_fwd"][1][i] is L._i
    assert {k: v for k, v in got.items() if v != base[k]} == \
        {"sepr_dynmix_fwd": (L._i, base["sepr_dynmix_fwd"][1][:i] + [L._i] + base["sepr_dynmix_fwd"][1][i + 1:])}
    # two swapped parameters swap
    assert "int n, long long count, float eps" in HDR
    got = derive(HDR.replace("int n, long long count, float eps", "long long count, int n, float eps"))
    a = base["sepr_groupnorm_stats"][1]
    assert a[1:3] == [L._i, L._ll] and {k: v for k, v in got.items() if v != base[k]} == {"sepr_groupnorm_stats": (L._i, [a[0], a[2], a[1]] + a[3:])}
    # an added enum member shifts the values after it, in its enum only
    e = abi.parse(HDR.replace("SEPR_OP_GCFN, SEPR_OP_CLA,", "SEPR_OP_GCFN, SEPR_OP_NEW, SEPR_OP_CLA,")).enums
    assert e["SEPR_OP_NEW"] == 2
    assert {k: v for k, v in e.items() if H.enums.get(k) != v} == \
        {"SEPR_OP_NEW": 2, **{k: H.enums[k] + 1 for k in ("SEPR_OP_CLA", "SEPR_OP_EGA", "SEPR_OP_SPKATTN", "SEPR_OP_SPKSPLIT",
                                                            "SEPR_OP_OUTLAYER", "SEPR_OP_PIT", "SEPR_OP_COUNT")}}


KNOB = "int sepr_knob(int id);"
OUTSIDE_THE_SUBSET = {
    "an unknown type": (KNOB, "int sepr_knob(wchar_t id);", "int sepr_knob(wchar_t"),
    "an unknown return type": (KNOB, "bool sepr_knob(int id);", "bool sepr_knob"),
    "an unnamed parameter": (KNOB, "int sepr_knob(int);", "int sepr_knob(int)"),
    "an unnamed pointer parameter": ("float* y, int n, int T, int F, const sepr_gcfn_w* w,", "float*, int n, int T, int F, const sepr_gcfn_w* w,", "float*, int n, int T"),
    "an unnamed two-word parameter": ("long long sepr_resample_out_len(long long T,", "long long sepr_resample_out_len(long long,", "long long sepr_resample_out_len(long long,"),
    "an unterminated struct": ("  const float* bias;\n} sepr_x3_w;", "  const float* bias;\n", "typedef struct {\n  const void* wp;"),
    "a stray statement": (KNOB, "int sepr_counter;\n" + KNOB, "int sepr_counter;"),
    "a function body": (KNOB, "int sepr_two(void) { return 2; }\n" + KNOB, "int sepr_two(void)"),
    "a stray directive": (KNOB, "#pragma pack(1)\n" + KNOB, "#pragma pack(1)"),
    "a conditional that could hide declarations": (KNOB, "#if 0\n" + KNOB + "\n#endif", "#if 0"),
    "a define that is no integer": (KNOB, "#define SEPR_PI 3.14\n" + KNOB, "#define SEPR_PI"),
    "an array member": ("  int maxlen;\n  sepr_x3_w x3_gate;", "  int maxlen[2];\n  sepr_x3_w x3_gate;", "  int maxlen[2];"),
    "a member without a semicolon": ("  const float* bias;\n} sepr_x3_w;", "  const float* bias\n} sepr_x3_w;", "typedef struct {\n  const void* wp;"),
    "an enum value that is no integer": ("SEPR_OP_ENCODER = 0,", "SEPR_OP_ENCODER = 1 << 2,", "SEPR_OP_ENCODER = 1 << 2,"),
    "an empty enum member": ("SEPR_OP_ENCODER = 0,", "SEPR_OP_ENCODER = 0, ,", "SEPR_OP_ENCODER = 0, ,"),
    "a name declared twice": (KNOB, KNOB + "\n" + KNOB.replace("int id", "int other"), "int sepr_knob(int other);"),
}


@pytest.mark.parametrize("what", sorted(OUTSIDE_THE_SUBSET))
def test_outside_the_subset_raises_with_the_line(what):
    old, new, at = OUTSIDE_THE_SUBSET[what]
    assert HDR.count(old) == 1
    text = HDR.replace(old, new)
    with pytest.raises(abi.HeaderError) as e:
        abi.parse(text)
    line = text.count("\n", 0, text.index(at) + len(at) - len(at.lstrip())) + 1
    assert f"line {line}:" in str(e.value), (line, str(e.value))


def test_unclosed_block_and_missing_block_raise():
    opening = HDR.count("\n", 0, HDR.index('extern "C" {')) + 1
    with pytest.raises(abi.HeaderError, match=f"line {opening}: .*never closed"):
        abi.parse(HDR[:HDR.rindex("#ifdef __cplusplus")])
    with pytest.raises(abi.HeaderError, match="no extern"):
        abi.parse("int sepr_version(void);\n")


def test_tables_that_disagree_with_the_header_raise():
    cls = abi.struct_classes(H, L._STRUCTS)
    with pytest.raises(abi.HeaderError, match="lenghts"):                     # a host array the entry does not have
        abi.signatures(H, cls, {**L._HOST_ARRAYS, "sepr_bss_eval_fwd": "lenghts"})
    with pytest.raises(abi.HeaderError, match="'sepr_bss_eval_fwd', 'S'"):    # a parameter that is no pointer
        abi.signatures(H, cls, {**L._HOST_ARRAYS, "sepr_bss_eval_fwd": "lengths S"})
    with pytest.raises(abi.HeaderError, match="sepr_no_entry"):
        abi.signatures(H, cls, {**L._HOST_ARRAYS, "sepr_no_entry": "x"})
    with pytest.raises(abi.HeaderError, match="sepr_lin"):                    # a struct of the header without a name here
        abi.struct_classes(H, {k: v for k, v in L._STRUCTS.items() if k != "sepr_lin"})
    with pytest.raises(abi.HeaderError, match="sepr_gone"):                   # and a name without a struct
        abi.struct_classes(H, {**L._STRUCTS, "sepr_gone": "Gone"})


def test_host_arrays_are_the_typed_pointers_and_nothing_else_is():
    """The table names 14 entries; a parameter is POINTER(scalar) exactly where the table names it."""
    assert len(L._HOST_ARRAYS) == 14
    named = {(e, p) for e, ps in L._HOST_ARRAYS.items() for p in ps.split()}
    typed = {(e, p) for e, (_, params) in H.protos.items() for (_, p), a in zip(params, L.SIGNATURES[e][1])
             if issubclass(a, C._Pointer) and not issubclass(a._type_, C.Structure)}
    assert named == typed and len(named) == 39
    assert L.SIGNATURES["sepr_train_pack_lin"][1][0] is L._fp                 # const void* const* src: a DEVICE table
    lengths = L.SIGNATURES["sepr_bss_eval_fwd"][1][3]                         # what the typing is for: ctypes converts an int array
    lengths.from_param((C.c_int * 2)(1, 2))                                   # and refuses an array of another element type
    with pytest.raises(TypeError):
        lengths.from_param((C.c_longlong * 2)(1, 2))


def test_a_missing_header_is_a_library_error(tmp_path, monkeypatch):
    """lib.py finds the header relative to the package; a copy of the package with no include/ beside it raises on import and names the path."""
    pkg = tmp_path / "abi_probe_pkg"
    pkg.mkdir()
    for name in ("lib.py", "abi.py"):
        shutil.copy(os.path.join(ROOT, "sepreformer_amd", name), pkg / name)
    (pkg / "__init__.py").write_text("")
    monkeypatch.syspath_prepend(str(tmp_path))
    try:
        with pytest.raises(RuntimeError) as e:
            importlib.import_module("abi_probe_pkg.lib")
    finally:
        for k in [k for k in sys.modules if k.startswith("abi_probe_pkg")]:
            del sys.modules[k]
    assert type(e.value).__name__ == "SeprLibraryError" and os.path.join(str(tmp_path), "include", "sepr.h") in str(e.value)
