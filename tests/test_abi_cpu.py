"""The binding is generated from include/ladcast_hip.h by ladcast_amd.abi: the reader reads every declaration, refuses what it does
not know, and what it reads is what the hand-written binding held before it (tests/golden/abi_signatures.json, recorded from that
binding: the letters of every argument of every entry point, and name, size and offset of every struct field)."""
import ctypes
import json
import os
import re

import pytest

from ladcast_amd import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "ladcast_amd", "libladcast_hip.so")
needs_lib = pytest.mark.skipif(not os.path.exists(LIB), reason="libladcast_hip.so is not built")

with open(abi.HEADER_PATH) as _f:
    HEADER = _f.read()
with open(os.path.join(ROOT, "tests", "golden", "abi_signatures.json")) as _f:
    GOLDEN = json.load(_f)

LETTERS = {ctypes.c_void_p: "P", ctypes.c_int: "I", ctypes.c_longlong: "L", ctypes.c_float: "F", ctypes.c_double: "D", ctypes.c_char_p: "S"}
LETTERS.update({ctypes.POINTER(cls): "*" + name for name, cls in abi.STRUCTS.items()})


def test_every_recorded_prototype_and_struct_is_unchanged():
    assert len(GOLDEN["entry_points"]) == 116 and len(GOLDEN["structs"]) == 9
    host_arrays = 0
    for name, (res, args) in GOLDEN["entry_points"].items():
        got_res, got_args = abi.SIGNATURES[name]
        got = [LETTERS[a] for a in got_args]
        want = args.split()
        host_arrays += want.count("H")  # a host int array: POINTER(c_int) in the hand-written binding, a void* like every pointer now
        assert LETTERS[got_res] == res and got == ["P" if a == "H" else a for a in want], name
    assert host_arrays == 3
    for name, fields in GOLDEN["structs"].items():
        cls = abi.STRUCTS[name]
        assert [[f, getattr(cls, f).size, getattr(cls, f).offset] for f, _ in cls._fields_] == fields, name
    assert [ctypes.sizeof(abi.STRUCTS[n]) for n in GOLDEN["structs"]] == [72, 120, 208, 48, 72, 168, 20, 12, 516]


def test_the_reader_misses_nothing():
    declared = set(re.findall(r"\b(ldc_[a-z0-9_]+)\s*\(", HEADER)) - {"ldc_act"}  # the loose scan of test_host_cpu.py
    assert declared == set(abi.SIGNATURES) and len(declared) == 116
    typedefs = re.findall(r"typedef\s+struct\s+(\w+)", HEADER)
    assert sorted(typedefs) == sorted(abi.STRUCTS) and len(typedefs) == 9
    for name in re.findall(r"\b(ldc_\w+)\s*\*", re.sub(r"/\*.*?\*/", " ", HEADER, flags=re.S)):  # every struct pointer of a prototype
        assert name in abi.STRUCTS, name
    for name, (res, args) in abi.SIGNATURES.items():  # and nothing but the scalar classes, void* and pointers to those nine
        assert res in LETTERS and all(a in LETTERS for a in args), name


@pytest.mark.parametrize("text, named", [
    ("int ldc_f(const float* x, size_t n, void* stream);", ["ldc_f", "`n`", "size_t"]),
    ("typedef struct ldc_s {\n  int n;\n  int a[LDC_NOPE];\n} ldc_s;", ["ldc_s", "`a`", "LDC_NOPE"]),
    ("int ldc_f(const ldc_nope* p, void* stream);", ["ldc_f", "`p`", "ldc_nope"]),
])
def test_the_reader_refuses_what_it_does_not_know(text, named):
    with pytest.raises(ValueError) as e:
        abi.parse(text)
    for word in named:
        assert word in str(e.value), (word, str(e.value))


def test_the_reader_takes_the_awkward_shapes():
    P, I, L = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong
    constants, structs, sigs = abi.parse(
        "#define LDC_N 3 /* a bound */\n#define LDC_NEG (-2)\nenum ldc_act { LDC_ACT_NONE = 0, LDC_ACT_SILU = 1 };\n"
        "typedef struct ldc_in { const float* p; int a[LDC_N], b; } ldc_in;\n"
        "typedef struct ldc_out {\n  ldc_in in; /* nested */\n  long long s[2];\n} ldc_out;\n"
        "int ldc_g(const float* const* pp, unsigned char* m,\n          long long* n, const ldc_out* d, double k);\n"
        "long long ldc_h(void);\nconst char* ldc_name(void);\n")
    assert constants == {"LDC_N": 3, "LDC_NEG": -2, "LDC_ACT_NONE": 0, "LDC_ACT_SILU": 1}
    assert sigs == {"ldc_g": (I, [P, P, P, ctypes.POINTER(structs["ldc_out"]), ctypes.c_double]), "ldc_h": (L, []),
                    "ldc_name": (ctypes.c_char_p, [])}
    assert structs["ldc_in"]._fields_ == [("p", P), ("a", I * 3), ("b", I)]
    assert structs["ldc_out"]._fields_ == [("in", structs["ldc_in"]), ("s", L * 2)]
    assert ctypes.sizeof(structs["ldc_out"]) == 24 + 16


@needs_lib
def test_constants_of_the_binding_are_the_headers():
    import ladcast_amd.hip as hip

    matched = 0
    for name, value in abi.CONSTANTS.items():
        mine = getattr(hip, name[len("LDC_"):], None)
        if mine is not None:
            assert mine == value and type(mine) is int, name
            matched += 1
    assert matched >= 34
    assert hip.ABI_VERSION == abi.CONSTANTS["LDC_ABI_VERSION"] == hip.lib.ldc_abi_version()


@needs_lib
def test_struct_sizes_are_the_compilers():
    lib = ctypes.CDLL(LIB)
    checked = []
    for name, cls in abi.STRUCTS.items():
        size_of = "ldc_sizeof_" + name[len("ldc_"):]
        if size_of in abi.SIGNATURES:
            fn = getattr(lib, size_of)
            fn.restype, fn.argtypes = abi.SIGNATURES[size_of]
            assert fn() == ctypes.sizeof(cls), name
            checked.append(name)
    assert len(checked) == 8 and "ldc_linear_small_problem" not in checked
    assert ctypes.sizeof(abi.STRUCTS["ldc_linear_small_problem"]) == 72  # five pointers and eight ints
