"""The C types of libboxfusion_hip.so, read from include/boxfusion_hip.h: the one place they are written.
An extension header (EXTENSION_HEADERS: include/boxfusion_objects.h, include/boxfusion_level.h) is read the same way: every reader
below takes `header`, the path it reads, and defaults to the core header.

The header is regular: an entry point is `ret bf_name(type name, ...);`, a struct is
`typedef struct { fields } bf_name;`, a constant is `#define BF_NAME value` or an enum member.  A few
regular expressions read those forms (this is no C parser); a type that the tables below do not hold,
or a constant's value that is no integer literal, raises and names the function, field or constant.
"""
import ctypes
import functools
import os
import re

_INCLUDE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include")
HEADER = os.path.join(_INCLUDE, "boxfusion_hip.h")
EXTENSION_HEADERS = (os.path.join(_INCLUDE, "boxfusion_objects.h"),      # each includes the core header
                     os.path.join(_INCLUDE, "boxfusion_level.h"))

_SCALAR = {"int": ctypes.c_int, "float": ctypes.c_float, "double": ctypes.c_double, "size_t": ctypes.c_size_t,
           "long long": ctypes.c_longlong, "int64_t": ctypes.c_int64, "int32_t": ctypes.c_int32}
_RETURN = {"int": ctypes.c_int, "size_t": ctypes.c_size_t, "const char*": ctypes.c_char_p, "void": None}


@functools.lru_cache(maxsize=None)
def _source(header=None):
    with open(header or HEADER) as f:
        return re.sub(r"/\*.*?\*/|//[^\n]*", " ", f.read(), flags=re.S)


def _ctype(decl, where, known, header=None):
    """the ctypes type of `decl`, a parameter's or field's text without its name"""
    decl = " ".join(decl.split())
    if "*" in decl:
        return ctypes.c_void_p
    if decl not in known:
        raise TypeError(f"{header or HEADER}: {where}: no ctypes mapping for {decl!r}")
    return known[decl]


def struct(name, header=None):
    """ctypes.Structure class of `typedef struct { ... } name;`, fields in the header's order (one class
    per struct and header, however the header is named in the call)"""
    return _struct(name, header or HEADER)


@functools.lru_cache(maxsize=None)
def _struct(name, path):
    header = path
    body = re.search(r"typedef\s+struct\s*\{([^{}]*)\}\s*%s\s*;" % re.escape(name), _source(header))
    if body is None:
        raise KeyError(f"{path}: no typedef struct {name}")
    fields = []
    for decl in filter(None, (d.strip() for d in body.group(1).split(";"))):
        # `type a, b[16]`: the type ends at the first space or `*` that only names follow
        m = re.fullmatch(r"(.*?[\s*])((?:\s*\w+(?:\[\d+\])?\s*,?)+)", decl, re.S)
        if m is None:
            raise TypeError(f"{path}: {name}: cannot read the field {decl!r}")
        base = m.group(1).strip()
        known = {base: struct(base, header)} if base.startswith("bf_") else _SCALAR    # an earlier struct by value
        for fname, dim in re.findall(r"(\w+)(?:\[(\d+)\])?", m.group(2)):
            t = _ctype(base, f"{name}.{fname}", known, header)
            fields.append((fname, t * int(dim) if dim else t))
    return type(name, (ctypes.Structure,), {"_fields_": fields})


@functools.lru_cache(maxsize=None)
def prototypes(header=None):
    """{entry point: (restype, [argtypes])} of every bf_* prototype that `header` itself declares"""
    path = header or HEADER
    out = {}
    for ret, name, params in re.findall(r"([\w \t*]+?)\s*\b(bf_\w+)\s*\(([^()]*)\)\s*;", _source(header)):
        ret = " ".join(ret.split())
        if ret not in _RETURN:
            raise TypeError(f"{path}: {name}: no ctypes mapping for the return type {ret!r}")
        params = [] if params.strip() in ("", "void") else params.split(",")
        # a parameter is `type name`; the name is dropped (a pointer's may touch its `*`)
        out[name] = (_RETURN[ret], [_ctype(re.sub(r"\w+\s*$", "", p), f"{name}, parameter {i + 1}", _SCALAR, header)
                                    for i, p in enumerate(params)])
    return out


# an integer literal (decimal or hex, u / l / ll suffixes), optionally `<<` a second one, optionally in parentheses
_LITERAL = r"(-?\s*(?:0[xX][0-9a-fA-F]+|\d+))[uUlL]{0,3}"
_VALUE = re.compile(r"%s(?:\s*<<\s*%s)?" % (_LITERAL, _LITERAL))


def _value(text, name, header=None):
    inner = text.strip()
    if inner.startswith("(") and inner.endswith(")"):
        inner = inner[1:-1].strip()
    m = _VALUE.fullmatch(inner)
    if m is None:
        raise ValueError(f"{header or HEADER}: {name}: cannot read the value {text.strip()!r}")
    v = int(m.group(1).replace(" ", ""), 0)
    return v << int(m.group(2), 0) if m.group(2) else v


def _enums(src, header=None):
    """[{member: int}] per enum body, in the header's order; a member without a value is the one before it plus one"""
    out = []
    for body in re.findall(r"\benum\b[^{;]*\{([^{}]*)\}", src):
        members, nxt = {}, 0
        for member in filter(None, (m.strip() for m in body.split(","))):
            name, _, text = member.partition("=")
            name = name.strip()
            members[name] = nxt = _value(text, name, header) if text else nxt
            nxt += 1
        out.append(members)
    return out


def constants(source=None, header=None):
    """{name: int} of every object-like `#define BF_NAME value` and every enum member that `header` itself
    holds (not those of a header it includes); `source`: header text to read instead of the file"""
    src = _source(header) if source is None else source
    out = {}
    for name, call, text in re.findall(r"^[ \t]*#[ \t]*define[ \t]+(BF_\w+)(\()?(.*)$", src, re.M):
        if not call:                                   # a function-like macro is no constant
            out[name] = _value(text, name, header)
    for members in _enums(src, header):
        out.update(members)
    return out


def enum_names(prefix, source=None, header=None):
    """the members of the one enum whose members all start with `prefix`, in value order, the prefix stripped
    and lower-cased: the names of a counter tensor's words from the enum of its indices"""
    found = [e for e in _enums(_source(header) if source is None else source, header)
             if e and all(k.startswith(prefix) for k in e)]
    if len(found) != 1:
        raise KeyError(f"{header or HEADER}: {len(found)} enums whose members all start with {prefix}")
    return tuple(k[len(prefix):].lower() for k in sorted(found[0], key=found[0].get))


def declare(lib, header=None):
    """set restype and argtypes on every entry point of the loaded library that `header` declares; with
    no header given, the core header's and then every extension header's"""
    for h in ((None,) + EXTENSION_HEADERS if header is None else (header,)):
        for name, (restype, argtypes) in prototypes(h).items():
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = restype, argtypes
    return lib
