"""Reader of this project's C headers (include/*.h): the ctypes binding is derived from the prototypes and typedefs
themselves instead of being kept as a second, positional copy of them.

The headers are restricted C: ``dvg_*`` function declarations, ``typedef struct { ... } dvg_*_t;`` with scalar, pointer and
array fields, opaque struct typedefs and ``typedef void *``.  Anything else is an error that names the header, the function
and the parameter: the reader never skips and never guesses.

Type mapping: a scalar maps by name to the exact-width ctypes type; a pointer to a scalar, to ``void`` or to an opaque type,
and an alias of ``void *``, map to ``c_void_p`` (callers pass addresses, ``None``, ``byref(...)`` and ctypes arrays);
``char *`` maps to ``c_char_p``; a pointer to a struct with a body maps to ``POINTER`` of the generated Structure, unless the
struct is one of ``DEVICE_STRUCTS`` (it lives in device memory and is passed as an address); a pointer to a
pointer maps to ``POINTER(c_void_p)``; an array parameter ``T x[N]`` is ``T *x``.
"""
from __future__ import annotations

import ctypes
import functools
import os
import re

INCLUDE_DIR = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include"))

SCALARS = {
    "int": ctypes.c_int, "int8_t": ctypes.c_int8, "uint8_t": ctypes.c_uint8, "int32_t": ctypes.c_int32,
    "int64_t": ctypes.c_int64, "uint32_t": ctypes.c_uint32, "uint64_t": ctypes.c_uint64, "float": ctypes.c_float,
    "double": ctypes.c_double, "size_t": ctypes.c_size_t,
}


# structs that live in device memory: a pointer to one crosses the boundary as an address, like any device pointer
DEVICE_STRUCTS = ("dvg_step_state_t",)


class DvgError(RuntimeError):
    pass


class Header:
    """``protos``: name -> (restype, [(param_name, ctype), ...]); ``layouts``: typedef name -> [(field, ctype, array_len)]
    (array_len 0: not an array); ``structures``: typedef name -> the ctypes.Structure generated from that layout."""

    def __init__(self, path):
        self.path = path
        self.protos, self.layouts, self.structures = {}, {}, {}
        self.inherited = {}  # layouts of the headers this one includes
        self.opaque = set()  # opaque struct typedefs and aliases of `void *`: only their addresses cross the boundary
        self.aliases = set()  # the aliases of `void *` among them


def _error(path, where, what):
    return DvgError(f"{os.path.basename(path)}: {where}: {what}")


def _declarator(hdr, where, text, base=None):
    """One declarator (``const float *const keep[4]``; with ``base``, a further one of a field list: ``*conv_b[4]``)
    -> (base type name, pointer depth, name, array_len)."""
    if re.search(r"[^\w\s*\[\]]", text):
        raise _error(hdr.path, where, f"cannot read the declarator {text.strip()!r}")
    m = re.fullmatch(r"(.*?)\s*(?:\[\s*(\d+)\s*\])?\s*", text, flags=re.S)
    tokens = [t for t in re.findall(r"\w+|\*|\[|\]", m.group(1)) if t != "const"]
    if "[" in tokens or "]" in tokens:
        raise _error(hdr.path, where, f"cannot read the declarator {text.strip()!r}")
    words = [t for t in tokens if t != "*"]
    if base is None:
        if not words:
            raise _error(hdr.path, where, f"no type in {text.strip()!r}")
        base, words = words[0], words[1:]
        if tokens[0] != base:
            raise _error(hdr.path, where, f"cannot read the declarator {text.strip()!r}")
        tokens = tokens[1:]
    if len(words) != 1 or tokens[-1] != words[0]:
        raise _error(hdr.path, where, f"expected '<type> [*...] <name>' in {text.strip()!r} (type {base!r})")
    return base, tokens.count("*"), words[0], int(m.group(2) or 0)


def _ctype(hdr, where, base, depth, by_address):
    structs = {**hdr.inherited, **hdr.layouts}
    known = base in SCALARS or base in hdr.opaque or base in structs or base in ("void", "char")
    if not known:
        raise _error(hdr.path, where, f"unknown type {base!r}")
    if base in hdr.aliases:
        depth += 1
    if depth == 0 and base in SCALARS:
        return SCALARS[base]
    if depth == 1 and base == "char":
        return ctypes.c_char_p
    if depth == 1 and base in structs and base not in by_address:
        return ctypes.POINTER(hdr.structures[base])
    if depth == 1 and base != "char":
        return ctypes.c_void_p
    if depth == 2 and base != "char" and base not in hdr.aliases:
        return ctypes.POINTER(ctypes.c_void_p)
    raise _error(hdr.path, where, f"no ctypes mapping for {base!r} at pointer depth {depth}")


def _struct(hdr, name, body, by_address):
    layout = []
    for line in body.split(";"):
        if not line.strip():
            continue
        base = None
        for piece in line.split(","):
            base, depth, field, n = _declarator(hdr, f"{name}", piece, base)
            layout.append((field, _ctype(hdr, f"{name}.{field}", base, depth, by_address), n))
    hdr.layouts[name] = layout
    hdr.structures[name] = type(name, (ctypes.Structure,), {"_fields_": [(f, t * n if n else t) for f, t, n in layout]})


def _prototype(hdr, ret, name, params, by_address):
    base, depth, _, n = _declarator(hdr, name, ret + " _")
    if n:
        raise _error(hdr.path, name, "array return type")
    restype = _ctype(hdr, f"{name} (return type)", base, depth, by_address)
    out = []
    if params.strip() != "void":
        for k, piece in enumerate(params.split(",")):
            base, depth, pname, n = _declarator(hdr, f"{name}, parameter {k + 1}", piece)
            out.append((pname, _ctype(hdr, f"{name}, parameter {pname!r}", base, depth + (1 if n else 0), by_address)))
    hdr.protos[name] = (restype, out)


def _statements(path, text):
    """The header's text without comments and preprocessor lines, split at the ``;`` outside braces."""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    lines = []
    for line in text.split("\n"):
        if line.rstrip().endswith("\\"):
            raise _error(path, "preprocessor", f"line continuation in {line.strip()!r}")
        lines.append("" if line.lstrip().startswith("#") else line)
    text = "\n".join(lines)
    if 'extern "C" {' in text:  # the one linkage block around the declarations: drop it and its closing brace
        text = text.replace('extern "C" {', "", 1)
        head, brace, tail = text.rpartition("}")
        if not brace or tail.strip():
            raise _error(path, 'extern "C"', "its closing brace is not the last token")
        text = head
    out, depth, start = [], 0, 0
    for i, ch in enumerate(text):
        depth += (ch == "{") - (ch == "}")
        if ch == ";" and depth == 0:
            out.append(text[start:i].strip())
            start = i + 1
    if depth or text[start:].strip():
        raise _error(path, "end of file", f"unterminated text {text[start:].strip()[:60]!r}")
    return [s for s in out if s]


def parse(text: str, path: str, by_address: tuple = DEVICE_STRUCTS) -> Header:
    """The prototypes and struct layouts of a header's text; ``path`` names it in errors."""
    hdr = Header(path)
    for inc in re.findall(r'^\s*#\s*include\s+"([^"]+)"', text, flags=re.M):
        other = read(inc)
        hdr.structures.update(other.structures)
        hdr.inherited.update(other.inherited, **other.layouts)
        hdr.opaque |= other.opaque
        hdr.aliases |= other.aliases
    for stmt in _statements(path, text):
        if m := re.fullmatch(r"typedef\s+struct\s*\{(.*)\}\s*(\w+)", stmt, flags=re.S):
            _struct(hdr, m.group(2), m.group(1), by_address)
        elif m := re.fullmatch(r"typedef\s+struct\s+\w+\s+(\w+)", stmt):
            hdr.opaque.add(m.group(1))
        elif m := re.fullmatch(r"typedef\s+void\s*\*\s*(\w+)", stmt):
            hdr.opaque.add(m.group(1))
            hdr.aliases.add(m.group(1))
        elif m := re.fullmatch(r"([\w\s*]+?)\b(dvg_\w+)\s*\((.*)\)", stmt, flags=re.S):
            _prototype(hdr, m.group(1), m.group(2), m.group(3), by_address)
        else:
            raise _error(path, "declaration", f"cannot read {' '.join(stmt.split())[:80]!r}")
    return hdr


@functools.lru_cache(maxsize=None)
def read(name: str) -> Header:
    """The prototypes and struct layouts of include/<name>.  A header that includes another of the project's headers sees
    that header's types (and shares its Structures), not its prototypes."""
    path = os.path.join(INCLUDE_DIR, name)
    if not os.path.isfile(path):
        raise _error(path, "open", f"header not found at {path}")
    with open(path) as f:
        return parse(f.read(), path)


def signatures(name: str) -> dict:
    """name -> (restype, [argtypes]) of every function include/<name> declares: the shape the binding assigns."""
    return {fn: (res, [t for _, t in params]) for fn, (res, params) in read(name).protos.items()}
