"""The C types of libboxfusion_hip.so, read from include/boxfusion_hip.h: the one place they are written.

The header is regular: an entry point is `ret bf_name(type name, ...);`, a struct is
`typedef struct { fields } bf_name;`.  A few regular expressions read those two forms (this is no C
parser); a type that the tables below do not hold raises and names the function or field.
"""
import ctypes
import functools
import os
import re

HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "boxfusion_hip.h")

_SCALAR = {"int": ctypes.c_int, "float": ctypes.c_float, "double": ctypes.c_double, "size_t": ctypes.c_size_t,
           "long long": ctypes.c_longlong, "int64_t": ctypes.c_int64, "int32_t": ctypes.c_int32}
_RETURN = {"int": ctypes.c_int, "size_t": ctypes.c_size_t, "const char*": ctypes.c_char_p, "void": None}


@functools.lru_cache(maxsize=None)
def _source():
    with open(HEADER) as f:
        return re.sub(r"/\*.*?\*/|//[^\n]*", " ", f.read(), flags=re.S)


def _ctype(decl, where, known):
    """the ctypes type of `decl`, a parameter's or field's text without its name"""
    decl = " ".join(decl.split())
    if "*" in decl:
        return ctypes.c_void_p
    if decl not in known:
        raise TypeError(f"{HEADER}: {where}: no ctypes mapping for {decl!r}")
    return known[decl]


@functools.lru_cache(maxsize=None)
def struct(name):
    """ctypes.Structure class of `typedef struct { ... } name;`, fields in the header's order"""
    body = re.search(r"typedef\s+struct\s*\{([^{}]*)\}\s*%s\s*;" % re.escape(name), _source())
    if body is None:
        raise KeyError(f"{HEADER}: no typedef struct {name}")
    fields = []
    for decl in filter(None, (d.strip() for d in body.group(1).split(";"))):
        # `type a, b[16]`: the type ends at the first space or `*` that only names follow
        m = re.fullmatch(r"(.*?[\s*])((?:\s*\w+(?:\[\d+\])?\s*,?)+)", decl, re.S)
        if m is None:
            raise TypeError(f"{HEADER}: {name}: cannot read the field {decl!r}")
        base = m.group(1).strip()
        known = {base: struct(base)} if base.startswith("bf_") else _SCALAR    # an earlier struct by value
        for fname, dim in re.findall(r"(\w+)(?:\[(\d+)\])?", m.group(2)):
            t = _ctype(base, f"{name}.{fname}", known)
            fields.append((fname, t * int(dim) if dim else t))
    return type(name, (ctypes.Structure,), {"_fields_": fields})


@functools.lru_cache(maxsize=None)
def prototypes():
    """{entry point: (restype, [argtypes])} of every bf_* prototype"""
    out = {}
    for ret, name, params in re.findall(r"([\w \t*]+?)\s*\b(bf_\w+)\s*\(([^()]*)\)\s*;", _source()):
        ret = " ".join(ret.split())
        if ret not in _RETURN:
            raise TypeError(f"{HEADER}: {name}: no ctypes mapping for the return type {ret!r}")
        params = [] if params.strip() in ("", "void") else params.split(",")
        # a parameter is `type name`; the name is dropped (a pointer's may touch its `*`)
        out[name] = (_RETURN[ret], [_ctype(re.sub(r"\w+\s*$", "", p), f"{name}, parameter {i + 1}", _SCALAR)
                                    for i, p in enumerate(params)])
    return out


def declare(lib):
    """set restype and argtypes on every declared entry point of the loaded library"""
    for name, (restype, argtypes) in prototypes().items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = restype, argtypes
    return lib
