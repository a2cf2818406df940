"""Reader of include/gsraster.h: the C ABI as data.  The header is the one place the ABI is written; _native.py derives its
symbol list, its restype / argtypes and its constants from what `header()` returns, and tests/arena_helpers.py its parameter table.

    functions  {name: (return type, [(ctype, parameter, is_pointer, is_const)])}   e.g. ("int", [("const float*", "means3D", True, True)])
    constants  {name: int}  every `#define GSR_X <integer>` (a `u` suffix allowed) and every enumerator, explicit or counted on
    structs    {name: [(ctype, field, array length or None)]}  every `typedef struct`

`ctype` maps a declared type to its ctypes type and raises on one it does not know: nothing defaults to int."""
import collections
import ctypes
import os
import re

HEADER_PATH = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "gsraster.h")

Abi = collections.namedtuple("Abi", "functions constants structs")

SCALARS = {"int": ctypes.c_int, "unsigned": ctypes.c_uint, "unsigned int": ctypes.c_uint, "float": ctypes.c_float,
           "double": ctypes.c_double, "size_t": ctypes.c_size_t, "long long": ctypes.c_longlong,
           **{f"{u}int{n}_t": getattr(ctypes, f"c_{u}int{n}") for u in ("", "u") for n in (8, 16, 32, 64)}}


def _declarator(text):
    """'const float* const* weights' -> ('const float* const*', 'weights', None);  'double total_ms[N]' -> ('double', 'total_ms', 'N')"""
    m = re.match(r"^(.*?)(\w+)(?:\s*\[\s*(\w+)\s*\])?$", " ".join(text.split()))
    if not m or not m.group(1).strip():
        raise ValueError(f"gsraster.h: cannot read the declaration {text!r}")
    return re.sub(r"\s*\*", "*", m.group(1).strip()), m.group(2), m.group(3)


def parse(text, scope=None):
    """The text of a header in gsraster.h's style -> Abi(functions, constants, structs).  scope: constants of another header that an
    array length here may name (an extension header read with the main header's in scope); they are not repeated in the result."""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    constants = {m.group(1): int(m.group(2), 0)
                 for m in re.finditer(r"^[ \t]*#[ \t]*define[ \t]+(GSR_\w+)[ \t]+(-?(?:0[xX][0-9a-fA-F]+|\d+))[uU]?[ \t]*$", text, flags=re.M)}
    text = re.sub(r"^[ \t]*#[^\n]*", " ", text, flags=re.M)
    text = re.sub(r'extern\s+"C"\s*\{', " ", text)

    def enum(m):
        value = -1
        for item in filter(None, (e.strip() for e in m.group(1).split(","))):
            name, _, explicit = (s.strip() for s in item.partition("="))
            value = int(re.sub(r"[uU]$", "", explicit), 0) if explicit else value + 1
            constants[name] = value
        return " "
    text = re.sub(r"(?:typedef\s+)?\benum\b[^{;]*\{(.*?)\}[^;]*;", enum, text, flags=re.S)

    structs = {}

    def struct(m):
        fields = structs[m.group(2)] = []
        for decl in filter(None, (d.strip() for d in m.group(1).split(";"))):
            first, *more = decl.split(",")
            ctype, name, length = _declarator(first)
            for name, length in [(name, length)] + [_declarator(ctype + " " + d)[1:] for d in more]:
                fields.append((ctype, name, None if length is None else int(length) if length.isdigit() else constants[length] if length in constants or not scope else scope[length]))
        return " "
    text = re.sub(r"typedef\s+struct\b[^{;]*\{(.*?)\}\s*(\w+)\s*;", struct, text, flags=re.S)

    functions = {}
    for m in re.finditer(r"([A-Za-z_][\w\s\*]*?)\b(gsr_\w+)\s*\(([^()]*)\)\s*;", text):
        params = []
        if m.group(3).strip() not in ("", "void"):
            for p in m.group(3).split(","):
                ctype, name, _ = _declarator(p)
                params.append((ctype, name, "*" in ctype, ctype.startswith("const ")))
        functions[m.group(2)] = (re.sub(r"\s*\*", "*", " ".join(m.group(1).split())), params)
    return Abi(functions, constants, structs)


_header = None


def header():
    """parse() of include/gsraster.h, read once per process.  A missing header is as fatal as a missing library: no fallback table."""
    global _header
    if _header is None:
        try:
            with open(HEADER_PATH) as f:
                text = f.read()
        except OSError as e:
            raise RuntimeError(f"gscream_amd: the C ABI header {HEADER_PATH} cannot be read ({e}); the binding is derived from it "
                               "and has no table of its own") from e
        _header = parse(text)
    return _header


_extensions = {}


def extension(name):
    """parse() of include/<name>, an extension family's header (gsraster_jpeg_decode.h), with header()'s constants in scope; read once
    per process.  header() itself -- the main header's functions, constants and structs -- is what it was."""
    if name not in _extensions:
        path = os.path.join(os.path.dirname(HEADER_PATH), name)
        try:
            with open(path) as f:
                text = f.read()
        except OSError as e:
            raise RuntimeError(f"gscream_amd: the C ABI header {path} cannot be read ({e}); the binding is derived from it") from e
        _extensions[name] = parse(text, header().constants)
    return _extensions[name]


def ctype(decl, structs=(), returns=False):
    """ctypes type of the declared type `decl`.  structs: {C struct name: ctypes.Structure class}; a pointer to one of them is
    POINTER(class), every other pointer (T* const* included) c_void_p.  returns=True reads a return type: `void` is None and the one
    pointer allowed is `const char*`.  A type that is not in the map raises TypeError."""
    if returns and decl in ("void", "const char*"):
        return None if decl == "void" else ctypes.c_char_p
    if "*" in decl and not returns:
        pointee = re.sub(r"\bconst\b", "", decl[:-1]).strip()
        return ctypes.POINTER(structs[pointee]) if pointee in structs else ctypes.c_void_p
    if decl not in SCALARS:
        raise TypeError(f"gsraster.h: no ctypes type is known for {decl!r}; add it to gscream_amd/_abi.py SCALARS")
    return SCALARS[decl]
