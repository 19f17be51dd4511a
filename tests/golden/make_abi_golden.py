#!/usr/bin/env python3
"""What ``sepreformer_amd/lib.py`` bound BEFORE the binding was derived from include/sepr.h (docs/HISTORY.md, "the C ABI").

    git show <parent commit>:sepreformer_amd/lib.py > /tmp/parent_lib.py
    python tests/golden/make_abi_golden.py --lib /tmp/parent_lib.py

Imports the PARENT commit's hand-written ``lib.py`` from the given file (never the tree under test: the script refuses to run without
``--lib``) and writes ``abi_binding.json``: per entry the return and argument types, per struct the fields with their types, offsets
and the size, and every constant.  ``tests/test_abi_cpu.py`` asserts that ``describe()`` of the derived binding is that record.
No library and no device are needed.

Types are written as the classes ctypes distinguishes: i, ll, sz (size_t and unsigned long long are one class on LP64), f, d, p
(c_void_p), s (c_char_p), v (None), P(x) = POINTER of a scalar class, P:Name = POINTER of a struct, S:Name = a struct member.
"""
from __future__ import annotations

import argparse
import ctypes as C
import importlib.util
import json
import os

HERE = os.path.dirname(os.path.abspath(__file__))
_CODES = [(C.c_int, "i"), (C.c_longlong, "ll"), (C.c_size_t, "sz"), (C.c_ulonglong, "u64"), (C.c_float, "f"), (C.c_double, "d"),
          (C.c_void_p, "p"), (C.c_char_p, "s")]


def code(t) -> str:
    if t is None:
        return "v"
    for cls, name in _CODES:
        if t is cls:
            return name
    if issubclass(t, C.Structure):
        return "S:" + t.__name__
    if issubclass(t, C._Pointer):
        return "P:" + t._type_.__name__ if issubclass(t._type_, C.Structure) else "P(" + code(t._type_) + ")"
    raise TypeError(f"a ctypes class the record has no name for: {t!r}")


def describe(L) -> dict:
    """The whole public binding of a ``lib`` module as plain data."""
    structs = {k: v for k, v in vars(L).items() if isinstance(v, type) and issubclass(v, C.Structure) and not k.startswith("_")}
    return {
        "entries": {name: [code(res), [code(a) for a in args]] for name, (res, args) in L.SIGNATURES.items()},
        "structs": {k: {"fields": [[f, code(t)] for f, t in v._fields_], "offsets": [getattr(v, f).offset for f, _ in v._fields_],
                        "size": C.sizeof(v)} for k, v in sorted(structs.items())},
        "constants": {k: v for k, v in sorted(vars(L).items()) if k.isupper() and isinstance(v, int) and not k.startswith("_")},
        "ledger_slots": dict(L.LEDGER_SLOTS),
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", required=True, help="the parent commit's sepreformer_amd/lib.py, saved to a file outside the tree")
    a = ap.parse_args()
    spec = importlib.util.spec_from_file_location("parent_lib", a.lib)
    L = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(L)
    if not hasattr(L, "_tstruct"):
        raise SystemExit(f"{a.lib} is not the hand-written binding: the golden record comes from the parent commit, not from the tree under test")
    rec = describe(L)
    path = os.path.join(HERE, "abi_binding.json")
    with open(path, "w") as f:
        f.write("{\n" + ",\n".join(f' "{sec}": {{\n' + ",\n".join(f"  {json.dumps(k)}: {json.dumps(v, separators=(',', ':'))}" for k, v in body.items())
                                   + "\n }" for sec, body in rec.items()) + "\n}\n")
    print(f"{path}: {len(rec['entries'])} entries, {len(rec['structs'])} structs, {len(rec['constants'])} constants from {a.lib}")


if __name__ == "__main__":
    main()
