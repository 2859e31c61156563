"""The one reader of include/msl.h and include/msl_debug.h: the declarations, records and integer constants the Python binding is built from.
Plain `re`; whatever it does not know it refuses, naming the culprit.  tests/test_abi.py checks its output against a C++ compiler."""
import ctypes as C
import functools
import os
import re

import numpy as np

INCLUDE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")


class MslError(RuntimeError):
    pass


# parameter and return types by value; there is no default
_SCALARS = {"int": C.c_int, "int32_t": C.c_int, "msl_mem": C.c_int, "unsigned": C.c_uint, "size_t": C.c_size_t, "float": C.c_float,
            "double": C.c_double, "long long": C.c_longlong}
_FIELDS = {"float": "<f4", "double": "<f8", "int32_t": "<i4", "uint8_t": "u1"}      # record members


def text(name):
    """The header `name` without its /* */ and // comments."""
    path = os.path.join(INCLUDE, name)
    if not os.path.exists(path):
        raise MslError(f"{path} is missing: the Python binding is read from the C headers, which ship beside the package.")
    with open(path) as f:
        return re.sub(r"/\*.*?\*/|//[^\n]*", " ", f.read(), flags=re.S)


_PARAM = re.compile(r"\s*([\w\s*]*[\s*])(\w+)\s*(\[\w*\])?\s*(?:,|$)")      # type text, name, array extent


@functools.lru_cache(maxsize=None)
def _type(t):
    return " ".join(t.replace("*", " * ").split())


def declarations(text):
    """name -> (return type, [(type text, parameter name), ...]) of every `MSL_API ... MSL_NOEXCEPT;` statement, in header order.  Type text is
    normalised (`const float *`, `msl_match *`), an array parameter keeps its extent (`const float[16]`)."""
    code = re.sub(r"^[ \t]*#.*$", "", text, flags=re.M)
    out = {}
    for stmt in re.findall(r"\bMSL_API\b([^;]*);", code):
        m = re.fullmatch(r"\s*([\w\s*]*[\s*])(\w+)\s*\((.*)\)\s*MSL_NOEXCEPT\s*", stmt, flags=re.S)
        if not m:
            raise MslError(f"cannot read `MSL_API{stmt};` as `MSL_API type name(parameters) MSL_NOEXCEPT;`")
        ret, name, params = m.groups()
        params = "" if params.strip() == "void" else params
        rest = _PARAM.sub("", params).strip()                    # what no `type name` or `type name[N]` consumed
        if rest:
            raise MslError(f"{name}: cannot read the parameter list at `{rest}`")
        out[name] = (_type(ret), [(_type(t) + ext, p) for t, p, ext in _PARAM.findall(params)])
    if len(out) != code.count("MSL_API"):
        raise MslError(f"{code.count('MSL_API')} MSL_API tokens but {len(out)} distinct declarations read")
    return out


def _ctype(t, where):
    base = t.replace("const ", "")
    if base == "char *":
        return C.c_char_p
    if "*" in t or "[" in t:
        return C.c_void_p
    if base not in _SCALARS:
        raise MslError(f"{where}: no ctypes rule for the type `{t}`")
    return _SCALARS[base]


def ctypes_of(declaration, name="?"):
    """(restype, argtypes) of one entry of declarations(); `name` is the function's, for the messages."""
    ret, args = declaration
    return (None if ret == "void" else _ctype(ret, f"{name}: return value"),
            [_ctype(t, f"{name}: parameter {p}") for t, p in args])


def defines(text):
    """name -> value of every `#define NAME <integer>`."""
    return {k: int(v) for k, v in re.findall(r"^[ \t]*#[ \t]*define[ \t]+(\w+)[ \t]+(-?\d+)[uU]?[ \t]*$", text, flags=re.M)}


def _walk(dt, base=0, path=""):
    for n in dt.names:
        sub, off = dt.fields[n][:2]
        if sub.names:
            yield from _walk(sub, base + off, path + n + ".")
        else:
            yield n, sub, base + off, path + n


def records(text):
    """struct name -> numpy dtype with C's layout, for every `typedef struct msl_x { ... } msl_x;`.  A member whose type is an earlier record is
    flattened in place under its inner field names; dtype.metadata["paths"] keeps each field's C member path (`base.fx`), in field order."""
    consts, nested, out = defines(text), {}, {}
    for name, body in re.findall(r"\btypedef\s+struct\s+(\w+)\s*\{(.*?)\}\s*\1\s*;", text, flags=re.S):
        members = []
        for stmt in filter(None, (s.strip() for s in body.split(";"))):
            ctype, items = (stmt.split(None, 1) + [""])[:2]
            fmt = nested.get(ctype, _FIELDS.get(ctype))
            if fmt is None:
                raise MslError(f"{name}: `{stmt}` has a type that is neither a known scalar nor an earlier record")
            for item in items.split(","):
                f = re.fullmatch(r"\s*(\w+)\s*(?:\[\s*(\w+)\s*\])?\s*", item)
                field, ext = f.groups() if f else (None, None)
                if ext is not None:                                      # an extent: a literal or a #define, and not of records
                    ext = int(ext) if ext.isdigit() else consts.get(ext)
                    field = field if ext and ctype not in nested else None
                if field is None:
                    raise MslError(f"{name}: cannot read member `{item.strip()}` of `{stmt}`")
                members.append((field, fmt) if ext is None else (field, fmt, (ext,)))
        nested[name] = np.dtype(members, align=True)
        rows = list(_walk(nested[name]))
        names = [r[0] for r in rows]
        if len(set(names)) != len(names):
            raise MslError(f"{name}: flattened members collide: {sorted(n for n in set(names) if names.count(n) > 1)}")
        out[name] = np.dtype({"names": names, "formats": [r[1] for r in rows], "offsets": [r[2] for r in rows], "itemsize": nested[name].itemsize},
                             align=True, metadata={"paths": tuple(r[3] for r in rows)})
    return out
