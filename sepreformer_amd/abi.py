"""Reader of ``include/sepr.h``: the C ABI is stated there once, and ``lib.py`` derives its ctypes binding from what this module returns.

A reader for the header's subset of C89 declarations, not a C parser.  Between ``extern "C" {`` and its closing brace it knows ``#define NAME
integer``, ``#ifdef __cplusplus`` / ``#endif``, ``typedef struct { members } name;``, ``typedef type name;``, ``enum { A = n, B, ... };`` and
prototypes, with comments of both kinds anywhere.  Anything else raises ``HeaderError`` with the line, as do a base type outside the type table and
an unnamed parameter: nothing is skipped.  Text outside the block (the include guard, ``#include``) is NOT read: a declaration put there is lost.
"""
import ctypes as C
import re
from typing import NamedTuple


class HeaderError(ValueError):
    pass


# the type table: every base type a declaration may use, and the ctypes class of a value of it
SCALARS = {"void": None, "char": C.c_char, "short": C.c_short, "int": C.c_int, "unsigned": C.c_uint, "unsigned char": C.c_ubyte,
           "long long": C.c_longlong, "unsigned long long": C.c_ulonglong, "size_t": C.c_size_t, "float": C.c_float, "double": C.c_double}
_WORDS = {w for t in SCALARS for w in t.split()} | {"const", "struct", "enum", "typedef"}
_STATEMENT = re.compile(r"([^;{}]*(?:\{[^{}]*\}[^;{}]*)?);")   # up to its ';', with at most one pair of braces


class Header(NamedTuple):
    defines: dict    # name -> int
    enums: dict      # member -> int, all enums (they are anonymous), in declaration order
    typedefs: dict   # name -> C type
    structs: dict    # name -> [(C type, field)], in declaration order
    protos: dict     # name -> (return C type, [(C type, parameter)])


def _pieces(s, base, sep):
    """(offset in the header of its first non-blank character, stripped piece) for the sep-separated pieces of s, which starts at base."""
    out = []
    for p in s.split(sep):
        out.append((base + len(p) - len(p.lstrip()), p.strip()))
        base += len(p) + 1
    return out


def _int(s):
    m = re.fullmatch(r"\(?\s*(-?\d+)\s*\)?", s)
    return int(m.group(1)) if m else None


def split_type(t, h):
    """(base type without const, typedefs resolved; pointer depth) of a C type as parse() spells it."""
    base, depth = " ".join(w for w in t.replace("*", " ").split() if w != "const"), t.count("*")
    if base in h.typedefs:
        base, more = split_type(h.typedefs[base], h)
        depth += more
    return base, depth


def parse(text: str) -> Header:
    """Read the header's text.  Raises HeaderError, naming the line, for whatever is outside the subset."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", lambda m: " " + "\n" * m.group().count("\n"), text, flags=re.S)   # a comment keeps its line breaks, so lines still count
    h = Header({}, {}, {}, {}, {})

    def fail(pos, what):
        raise HeaderError(f"sepr.h line {text.count(chr(10), 0, pos) + 1}: {what}")

    def ctype(t, pos):
        t = " ".join(t.split()).replace(" *", "*")
        if split_type(t, h)[0] not in SCALARS and split_type(t, h)[0] not in h.structs:
            fail(pos, f"unknown type {t!r}")
        return t

    def decl(piece, pos):
        m = re.fullmatch(r"(.*?)(\w+)", piece, re.S)
        if not m or not m.group(1).strip() or m.group(2) in _WORDS:
            fail(pos, f"no name in {piece!r} (an unnamed parameter?)")
        t = ctype(m.group(1), pos)
        if split_type(t, h) == ("void", 0):
            fail(pos, f"{m.group(2)} is a void value")
        return t, m.group(2)

    def put(table, name, value, pos):
        if name in table:
            fail(pos, f"{name} is declared twice")
        table[name] = value

    start = re.search(r'extern\s+"C"\s*\{', text)
    if not start:
        raise HeaderError('sepr.h: no extern "C" { block')
    pos = start.end()
    while True:
        pos = re.compile(r"\s*").match(text, pos).end()
        if pos >= len(text):
            fail(start.start(), 'extern "C" { is never closed')
        if text[pos] == "}":
            return h
        if text[pos] == "#":
            end = text.find("\n", pos)
            end = len(text) if end < 0 else end
            d = text[pos:end].split()
            if d[0] == "#define" and len(d) == 3 and _int(d[2]) is not None:
                put(h.defines, d[1], _int(d[2]), pos)
            elif " ".join(d) not in ("#ifdef __cplusplus", "#endif"):      # (a general #if could hide what follows from the compiler only)
                fail(pos, f"unrecognised directive {text[pos:end].strip()!r}")
            pos = end
            continue
        m = _STATEMENT.match(text, pos)
        if not m:
            fail(pos, "a statement that does not end or nests braces (an unterminated struct or enum, a missing ';')")
        s, end = m.group(1), m.end(1)
        if st := re.fullmatch(r"typedef\s+struct\s*\{(.*)\}\s*(\w+)\s*", s, re.S):
            members = _pieces(st.group(1), pos + st.start(1), ";")
            if members.pop()[1]:
                fail(pos, f"the last member of {st.group(2)} has no ';'")
            fields = []
            for off, memb in members:
                first, *more = _pieces(memb, off, ",")      # several declarators share the first one's type
                t, name = decl(first[1], first[0])
                for o, n in [(first[0], name)] + more:
                    if not re.fullmatch(r"\w+", n) or n in _WORDS or n in [f for _, f in fields]:
                        fail(o, f"bad or repeated field name {n!r} in {st.group(2)}")
                    fields.append((t, n))
            put(h.structs, st.group(2), fields, pos)
        elif en := re.fullmatch(r"enum\s*\{(.*)\}\s*", s, re.S):
            value = 0
            for off, memb in _pieces(en.group(1).rstrip().removesuffix(","), pos + en.start(1), ","):    # (one trailing comma is C)
                m = re.fullmatch(r"(\w+)(?:\s*=\s*(.+))?", memb, re.S)
                if not m or (m.group(2) and _int(m.group(2)) is None):
                    fail(off, f"unrecognised enum member {memb!r}")
                value = _int(m.group(2)) if m.group(2) else value
                put(h.enums, m.group(1), value, off)
                value += 1
        elif "{" in s:
            fail(pos, "unrecognised statement with a brace")
        elif td := re.fullmatch(r"typedef\s+(.*?)(\w+)\s*", s, re.S):
            put(h.typedefs, td.group(2), ctype(td.group(1), pos), pos)
        elif (fn := re.fullmatch(r"(.*?)(\w+)\s*\((.*)\)\s*", s, re.S)) and fn.group(1).strip():
            params = _pieces(fn.group(3), pos + fn.start(3), ",")
            args = [] if [p for _, p in params] == ["void"] else [decl(p, o) for o, p in params]
            put(h.protos, fn.group(2), (ctype(fn.group(1), pos), args), pos)
        else:
            fail(pos, f"unrecognised statement {' '.join(s.split())[:60]!r}")
        pos = end + 1


def struct_classes(h: Header, names: dict) -> dict:
    """C struct name -> ctypes.Structure subclass called names[C name].  Any pointer is c_void_p (device pointers travel as plain
    addresses), a struct-typed member is its class, a scalar maps by the type table.  names must cover exactly the header's structs."""
    if set(names) != set(h.structs):
        raise HeaderError(f"the struct name map and sepr.h differ on {sorted(set(names) ^ set(h.structs))}")
    cls = {}
    for cname, fields in h.structs.items():
        ft = []
        for t, f in fields:
            base, depth = split_type(t, h)
            ft.append((f, C.c_void_p if depth else cls[base] if base in cls else SCALARS[base]))
        cls[cname] = type(names[cname], (C.Structure,), {"_fields_": ft})
    return cls


def signatures(h: Header, cls: dict, host_arrays: dict) -> dict:
    """entry -> (restype, argtypes).  ``const char*`` returns are c_char_p and void is None; a pointer to one struct is POINTER(its
    class); a parameter named in host_arrays[entry] (names separated by blanks) is a host array, POINTER(its element's class), so that
    ctypes refuses an array of another type; every other pointer is c_void_p; scalars map by the type table."""
    host = {(e, p) for e, ps in host_arrays.items() for p in ps.split()}
    pointers = {(e, p) for e, (_, params) in h.protos.items() for t, p in params if split_type(t, h)[1]}
    if host - pointers:
        raise HeaderError(f"host arrays that are no pointer parameter of sepr.h: {sorted(host - pointers)}")

    def one(t, is_host):
        base, depth = split_type(t, h)
        if depth == 1 and base in cls:
            return C.POINTER(cls[base])
        if depth:
            return C.POINTER(C.c_void_p if depth > 1 else SCALARS[base]) if is_host else C.c_void_p
        if base not in SCALARS:
            raise HeaderError(f"{t!r} is passed by value")
        return SCALARS[base]

    return {name: (C.c_char_p if ret == "const char*" else one(ret, False), [one(t, (name, p) in host) for t, p in params])
            for name, (ret, params) in h.protos.items()}
