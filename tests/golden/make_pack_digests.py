#!/usr/bin/env python3
"""What the inference packer produced BEFORE its weight forms were stated once (docs/HISTORY.md, "packed weight forms").

    git show <parent commit>:sepreformer_amd/pack.py > /tmp/parent_pack.py
    python tests/golden/make_pack_digests.py --pack /tmp/parent_pack.py --section cpu
    python tests/golden/make_pack_digests.py --pack /tmp/parent_pack.py --section device        # on the MI355X

Builds ``PackedModel`` with the PARENT commit's ``pack.py`` (never the tree under test: the script refuses to run without ``--pack``)
over synthetic weights and writes one section of ``pack_digests.json``: per row (variant, precision, one switch at most) one SHA-256,
truncated to 16 hex digits, per block struct, keyed by the struct's path in the model.  ``tests/test_pack_digests_cpu.py`` and
``tests/test_pack_digests_gpu.py`` assert that the tree's own ``pack.py`` gives every one of them.

A struct's digest runs over its fields in field order, nested structs included: a pointer as dtype, shape and bytes of the kept tensor
that starts at that address, a null pointer as a marker, ``maxlen`` as its value.  A switch row sets one of the switches ``pack.py``
reads to its non-default value on the variant where it matters and records only the structs that then differ from the plain row
(``differs``); all the others must equal the plain row's.
"""
from __future__ import annotations

import argparse
import contextlib
import ctypes as C
import hashlib
import importlib.util
import json
import os
import re
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from sepreformer_amd.config import VARIANTS  # noqa: E402
from sepreformer_amd.synth import synth_state_dict  # noqa: E402

PATH = os.path.join(HERE, "pack_digests.json")
SEED = 5
BASE, LARGE = "SepReformer_Base_WSJ0", "SepReformer_Large_DM_WHAMR"
ROWS = {"cpu": [(v, p) for v in ("tiny", "tiny3", BASE, LARGE) for p in ("fp32", "bf16x3")],     # F = 64, 64 with S = 3, 128, 256
        "device": [(v, "bf16x3") for v in ("tiny", BASE, LARGE)]}
# every switch pack.py reads -> (non-default value, variant on which it decides something)
SWITCHES = {"SEPR_FUSE_GCFN": ("0", BASE), "SEPR_FUSE_SPK": ("0", BASE), "SEPR_FUSE_CLA": ("0", BASE), "SEPR_FUSE_GATE": ("0", BASE),
            "SEPR_FUSE_MLP": ("0", BASE), "SEPR_FOLD_HEAD": ("0", BASE), "SEPR_FUSE_QKV": ("0", BASE), "SEPR_FUSE_OUT": ("0", BASE),
            "SEPR_FUSE_MLP256": ("1", LARGE), "SEPR_FUSE_GCFN256": ("0", LARGE), "SEPR_FUSE_CLA256": ("0", LARGE),
            "SEPR_FUSE_GATE256": ("0", LARGE), "SEPR_FUSE_SPK256": ("0", LARGE)}


def switches_named_in(pack_source: str):
    return sorted(set(re.findall(r"SEPR_[A-Z0-9_]+", pack_source)))


def load_pack(path: str):
    """``pack.py`` at ``path`` as a module of the ``sepreformer_amd`` package (its relative imports resolve to this tree's lib / config)."""
    spec = importlib.util.spec_from_file_location("sepreformer_amd._recorded_pack", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@contextlib.contextmanager
def only_switch(env: dict):
    """No switch of ``SWITCHES`` set except those of ``env``."""
    saved = {k: os.environ.pop(k, None) for k in SWITCHES}
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def _digest(items, by_ptr) -> str:
    """``items``: (ctypes type or None, value) in field order."""
    h = hashlib.sha256()
    for typ, v in items:
        if typ is C.c_int:
            h.update(b"int %d;" % v)
        elif not v:
            h.update(b"null;")
        else:
            t = by_ptr[v]
            h.update(f"{t.dtype} {tuple(t.shape)};".encode())
            h.update(t.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes())
    return h.hexdigest()[:16]


def _fields(st):
    for name, typ in st._fields_:
        v = getattr(st, name)
        if isinstance(v, C.Structure):
            yield from _fields(v)
        else:
            yield typ, v


def model_digests(pm) -> dict:
    """path -> digest for every block struct of a ``PackedModel``, the gate-perm pointers, the front-end tensors and the pe_k planes."""
    by_ptr = {}
    for t in pm.keep:
        u = by_ptr.setdefault(t.data_ptr(), t)
        if u is not t and (u.dtype, tuple(u.shape)) != (t.dtype, tuple(t.shape)):
            raise RuntimeError(f"two kept tensors of different form start at one address: {tuple(u.shape)} / {tuple(t.shape)}")
    out = {}

    def st(key, s):
        out[key] = _digest(_fields(s), by_ptr)

    def stage(p, d):
        for j, (ega, gcfn, perm) in enumerate(d["g"]):
            st(f"{p}.g.{j}.ega", ega)
            st(f"{p}.g.{j}.gcfn", gcfn)
            out[f"{p}.g.{j}.gate_perm"] = _digest([(None, perm)], by_ptr)
        for j, (cla, gcfn) in enumerate(d["l"]):
            st(f"{p}.l.{j}.cla", cla)
            st(f"{p}.l.{j}.gcfn", gcfn)
        for j, (mha, gcfn) in enumerate(d.get("spk", [])):
            st(f"{p}.spk.{j}.mha", mha)
            st(f"{p}.spk.{j}.gcfn", gcfn)
        if d.get("down") is not None:
            st(f"{p}.down", d["down"])

    for name in ("enc_w", "proj_g", "proj_b", "proj_w"):
        out["front." + name] = _digest([(None, getattr(pm, name))], by_ptr)
    ega0 = pm.enc_stages[0]["g"][0][0]
    out["pe_k"] = _digest([(None, ega0.pe_k)], by_ptr)
    out["pe_k_planes"] = _digest([(None, ega0.pe_k_planes)], by_ptr)
    for i, d in enumerate(pm.enc_stages):
        stage(f"enc_stages.{i}", d)
    stage("bottleneck", pm.bottleneck)
    for i, d in enumerate(pm.dec_stages):
        stage(f"dec_stages.{i}", d)
    for name in ("splits", "fuse", "out_aux"):
        for i, s in enumerate(getattr(pm, name)):
            st(f"{name}.{i}", s)
    st("out_main", pm.out_main)
    return out


_SD = {}


def digests_of(pack, variant: str, precision: str, device: str, env: dict) -> dict:
    if (variant, device) not in _SD:
        _SD[variant, device] = {k: v.to(device) for k, v in synth_state_dict(VARIANTS[variant], SEED).items()}   # moved first, as Model does
    with only_switch(env):
        return model_digests(pack.PackedModel(VARIANTS[variant], _SD[variant, device], precision))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pack", help="the PARENT commit's pack.py")
    ap.add_argument("--section", choices=("cpu", "device"), default="cpu")
    ap.add_argument("--out", default=PATH)
    a = ap.parse_args()
    if not a.pack:
        raise SystemExit("give --pack <the parent commit's pack.py>: the recording comes from the parent, not from the tree under test")
    pack = load_pack(a.pack)
    with open(a.pack) as f:
        named = switches_named_in(f.read())
    if named != sorted(SWITCHES):
        raise SystemExit(f"switches read by {a.pack}: {named}; recorded: {sorted(SWITCHES)}")
    dev = "cpu" if a.section == "cpu" else "cuda:0"
    rows, plain = [], {}
    for variant, precision in ROWS[a.section]:
        plain[variant, precision] = d = digests_of(pack, variant, precision, dev, {})
        rows.append({"variant": variant, "precision": precision, "env": {}, "digests": d})
    if a.section == "cpu":
        for name, (value, variant) in SWITCHES.items():
            d, ref = digests_of(pack, variant, "bf16x3", dev, {name: value}), plain[variant, "bf16x3"]
            assert sorted(d) == sorted(ref)
            differs = {k: v for k, v in d.items() if v != ref[k]}
            if not differs:
                raise SystemExit(f"{name}={value} changes nothing on {variant}")
            rows.append({"variant": variant, "precision": "bf16x3", "env": {name: value}, "differs": differs})
    doc = {}
    if os.path.exists(a.out):
        with open(a.out) as f:
            doc = json.load(f)
    doc[a.section] = rows
    with open(a.out, "w") as f:
        f.write("{\n" + ",\n".join(f' "{sec}": [\n' + ",\n".join("  " + json.dumps(r, separators=(",", ":")) for r in doc[sec]) + "\n ]"
                                   for sec in sorted(doc)) + "\n}\n")
    print(f"{a.out}: section {a.section}, {len(rows)} rows, {sum(len(r.get('digests', r.get('differs'))) for r in rows)} digests, seed {SEED}")


if __name__ == "__main__":
    main()
