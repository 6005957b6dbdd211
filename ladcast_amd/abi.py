"""The C ABI as ``include/ladcast_hip.h`` declares it, read from the header itself: constants, struct layouts and prototypes.
``include/ladcast_hip_ext.h``, the header of the entry points added after the recorded set of the first one, is read the same way into
``EXT_CONSTANTS`` and ``EXT_SIGNATURES``; it declares no struct, and a name it shares with the first header raises at import.

``ladcast_amd.hip`` builds its ctypes binding from this, so the header is the only place an entry point is declared.  The reader is
strict: a type it does not know, a statement it cannot split or an array bound it cannot resolve raises at import and names the item.
Nothing here imports torch or loads the library.
"""
import ctypes
import os
import re

HEADER_PATH = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "ladcast_hip.h"))
EXT_HEADER_PATH = os.path.join(os.path.dirname(HEADER_PATH), "ladcast_hip_ext.h")

_SCALARS = {"int": ctypes.c_int, "long long": ctypes.c_longlong, "float": ctypes.c_float, "double": ctypes.c_double}
_NAME = r"[A-Za-z_]\w*"


def _ctype(ctype, structs, where):
    """ctypes class of one C type; `structs`: the classes a struct pointer (or a field of struct type) may name"""
    t = " ".join(re.sub(r"\bconst\b", " ", ctype).replace("*", " * ").split())
    base, star, rest = t.partition(" *")
    if base in structs and not rest:  # the struct itself (a field of struct type), or a pointer to it
        return ctypes.POINTER(structs[base]) if star else structs[base]
    if base.startswith("ldc_") or not (star or base in _SCALARS):
        raise ValueError(f"{where}: unknown type `{ctype.strip()}`")
    return ctypes.c_void_p if star else _SCALARS[base]


def parse(text):
    """(constants, structs, signatures) of a header text: name -> int, C struct name -> generated ctypes.Structure,
    entry point -> (restype, [argtypes])"""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    constants = {}
    for name, value in re.findall(r"^[ \t]*#[ \t]*define[ \t]+(LDC_\w+)\b(.*)$", text, re.M):
        if not re.fullmatch(r"\s*(\(\s*-?\d+\s*\)|-?\d+)\s*", value):
            raise ValueError(f"{name}: `#define {name}{value}` is not an integer")
        constants[name] = int(value.strip(" \t()"))
    for body in re.findall(r"\benum\s+ldc_act\s*\{(.*?)\}\s*;", text, re.S):
        for item in body.split(","):
            m = re.fullmatch(rf"\s*({_NAME})\s*=\s*(-?\d+)\s*", item)
            if not m:
                raise ValueError(f"ldc_act: cannot read the enumerator `{item.strip()}`")
            constants[m[1]] = int(m[2])
    text = re.sub(r"^[ \t]*#[^\n]*$|\benum\s+ldc_act\s*\{[^}]*\}\s*;|\bextern\s+\"C\"\s*\{|^\}[ \t]*$", " ", text, flags=re.M)

    structs = {}

    def struct(m):
        name, fields = m[1], []
        for decl in filter(None, (d.strip() for d in m[2].split(";"))):
            f = re.fullmatch(rf"(.*?[\s*])((?:{_NAME}(?:\[\w+\])?\s*,\s*)*{_NAME}(?:\[\w+\])?)", decl, re.S)
            if not f:
                raise ValueError(f"{name}: cannot split the field `{decl}`")
            ctype = ctypes.c_void_p if "*" in f[1] else _ctype(f[1], structs, f"{name}: field `{decl}`")
            for field, bound in re.findall(rf"({_NAME})(?:\[(\w+)\])?", f[2]):
                if bound and not (bound.isdigit() or bound in constants):
                    raise ValueError(f"{name}: field `{field}` has the unresolved array bound `{bound}`")
                fields.append((field, ctype * (int(bound) if bound.isdigit() else constants[bound]) if bound else ctype))
        structs[name] = type(name, (ctypes.Structure,), {"_fields_": fields})
        return " "

    text = re.sub(rf"\btypedef\s+struct\s+({_NAME})\s*\{{(.*?)\}}\s*\1\s*;", struct, text, flags=re.S)

    signatures = {}
    for stmt in filter(None, (s.strip() for s in text.split(";"))):
        m = re.fullmatch(rf"(.*?[\s*])({_NAME})\s*\((.*)\)", stmt, re.S)
        if not m:
            raise ValueError(f"cannot split the statement `{' '.join(stmt.split())}` into a prototype")
        name, params = m[2], m[3].strip()
        args = []
        for p in [] if params == "void" else params.split(","):
            a = re.fullmatch(rf"(.*?[\s*])({_NAME})", p.strip(), re.S)
            if not a:
                raise ValueError(f"{name}: cannot split the parameter `{p.strip()}`")
            args.append(_ctype(a[1], structs, f"{name}: parameter `{a[2]}`"))
        ret = " ".join(m[1].split())
        signatures[name] = (ctypes.c_char_p if ret == "const char*" else _ctype(ret, {}, f"{name}: return"), args)
    return constants, structs, signatures


def _read(path=HEADER_PATH):
    if not os.path.exists(path):
        raise RuntimeError(f"{path} is missing: ladcast_amd.hip derives its binding of libladcast_hip.so from this header.")
    with open(path) as f:
        return f.read()


CONSTANTS, STRUCTS, SIGNATURES = parse(_read())


def _parse_ext():
    constants, structs, signatures = parse(_read(EXT_HEADER_PATH))
    shared = sorted((set(constants) & set(CONSTANTS)) | (set(signatures) & set(SIGNATURES)))
    if structs or shared:
        raise ValueError(f"{EXT_HEADER_PATH}: declares structs {sorted(structs)} / repeats {shared} of ladcast_hip.h; it takes flat arguments and new names only")
    return constants, signatures


EXT_CONSTANTS, EXT_SIGNATURES = _parse_ext()
