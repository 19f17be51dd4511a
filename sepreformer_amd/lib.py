"""ctypes binding of ``libsepr_hip.so`` (C ABI declared in ``include/sepr.h``).

The library is built in-tree by ``__graft_entry__.build()`` (``make -C sepreformer_amd/csrc``).  There is no
fallback of any kind: if the shared object is missing or an entry point fails, this module raises.
ctypes releases the GIL around every foreign call, so ``torch.nn.parallel.data_parallel`` replicas
(one Python thread per device, reference ``engine.py:64``) can drive the library concurrently.
"""
from __future__ import annotations

import ctypes as C
import os
import threading
from typing import Optional

from . import abi

_HERE = os.path.dirname(os.path.abspath(__file__))
# SEPR_LIB_VARIANT=<tag> loads a hand-built second library _native/libsepr_hip_<tag>.so for an A/B (tools/README.md); unset = the product library
_VARIANT = os.environ.get("SEPR_LIB_VARIANT", "")
LIB_PATH = os.path.join(_HERE, "_native", f"libsepr_hip_{_VARIANT}.so" if _VARIANT else "libsepr_hip.so")


class SeprLibraryError(RuntimeError):
    pass


# The C ABI is stated once, in include/sepr.h; everything from here to SIGNATURES is derived from it (abi.py), read once at import.
_HEADER = os.path.join(os.path.dirname(_HERE), "include", "sepr.h")
try:
    with open(_HEADER) as _f:
        _H = abi.parse(_f.read())
except OSError as e:
    raise SeprLibraryError(f"{_HEADER} is missing or unreadable ({e}): the ctypes binding is derived from it") from e

ABI_VERSION = _H.defines["SEPR_VERSION"]
SEPR_OK, SEPR_EINVAL, SEPR_EWORKSPACE, SEPR_EHIP = (_H.defines[k] for k in ("SEPR_OK", "SEPR_EINVAL", "SEPR_EWORKSPACE", "SEPR_EHIP"))
_ERR = {SEPR_EINVAL: "SEPR_EINVAL (bad shape / unsupported size / null pointer)", SEPR_EWORKSPACE: "SEPR_EWORKSPACE (workspace too small)",
        SEPR_EHIP: "SEPR_EHIP (HIP launch failed)"}

# module attributes OP_* (sepr_workspace_bytes), SITE_* (the kernel timer), TOP_* (the training sizes), KNOB_*: L.OP_GCFN is the header's SEPR_OP_GCFN
globals().update({k[5:]: v for k, v in _H.enums.items()
                  if k.startswith(("SEPR_OP_", "SEPR_SITE_", "SEPR_TOP_", "SEPR_KNOB_")) and not k.endswith("_COUNT")})
LEDGER_MAX_PARTS = _H.enums["SEPR_LEDGER_MAX_PARTS"]
LEDGER_SLOTS = {k[12:].lower(): v for k, v in _H.enums.items() if k.startswith("SEPR_LEDGER_") and k != "SEPR_LEDGER_MAX_PARTS"}   # the run ledger


def ledger_doubles(nparts: int) -> int:
    """Length of a ledger of ``nparts`` loss parts: the fixed slots, the sum of each part, the last step's parts."""
    return LEDGER_SLOTS["part_sum"] + 2 * int(nparts)


# the scalar classes by the names call sites build host arrays with; device pointers travel as plain addresses
_fp, _i, _f, _sz, _ll, _u64, _d = C.c_void_p, C.c_int, C.c_float, C.c_size_t, C.c_longlong, C.c_ulonglong, C.c_double

# every struct of the header and the name of its ctypes class, a module attribute (L.GcfnW); import raises if map and header differ
_STRUCTS = {"sepr_x3_w": "X3W", "sepr_gcfn_w": "GcfnW", "sepr_cla_w": "ClaW", "sepr_mha_w": "MhaW", "sepr_ega_w": "EgaW",
            "sepr_down_w": "DownW", "sepr_split_w": "SplitW", "sepr_fuse_w": "FuseW", "sepr_out_w": "OutW", "sepr_lin": "Lin",
            "sepr_gcfn_tw": "GcfnTW", "sepr_gcfn_grad": "GcfnGrad", "sepr_cla_tw": "ClaTW", "sepr_cla_grad": "ClaGrad",
            "sepr_mha_tw": "MhaTW", "sepr_mha_grad": "MhaGrad", "sepr_ega_tw": "EgaTW", "sepr_ega_grad": "EgaGrad",
            "sepr_down_tw": "DownTW", "sepr_down_grad": "DownGrad", "sepr_split_tw": "SplitTW", "sepr_split_grad": "SplitGrad",
            "sepr_fuse_tw": "FuseTW", "sepr_fuse_grad": "FuseGrad", "sepr_out_tw": "OutTW", "sepr_out_grad": "OutGrad",
            "sepr_front_tw": "FrontTW", "sepr_front_grad": "FrontGrad", "sepr_adamw_tables": "AdamWTables"}
_CLASSES = abi.struct_classes(_H, _STRUCTS)
globals().update({cls.__name__: cls for cls in _CLASSES.values()})

# The one thing the header cannot say: which pointers to scalars or to pointers are HOST arrays (read before the call returns).  They are
# typed POINTER(element), so that ctypes refuses an array of another type; the element type is the header's.  Keyed by entry and
# PARAMETER NAME; import raises for a name that is no pointer parameter of its entry.  Every other pointer is a device address.
_CONV = "conv_taps conv_L conv_M conv_K"
_HOST_ARRAYS = {
    "sepr_aux_decoder_fwd": "o2 idx wdec wav Tsrc", "sepr_bss_eval_fwd": "lengths", "sepr_stitch_fwd": "chunk_offset lengths",
    "sepr_streambank_step": "win", "sepr_streambank_convert": _CONV, "sepr_resample_fwd": "in_offset out_offset",
    "sepr_dynmix_fwd": "src", "sepr_dynmix_speed_fwd": "src " + _CONV, "sepr_dynmix_reverb_fwd": "src",
    "sepr_dynmix_speed_reverb_fwd": "src " + _CONV, "sepr_dynmix_turns_fwd": "src " + _CONV,
    "sepr_graph_pit_assign": "est rows", "sepr_graph_pit_assemble": "rows out", "sepr_prof_stop": "launches total_ms flops"}

# name -> (restype, argtypes) of every entry include/sepr.h declares
SIGNATURES = abi.signatures(_H, _CLASSES, _HOST_ARRAYS)

_lib: Optional[C.CDLL] = None
_lock = threading.Lock()


def load() -> C.CDLL:
    """dlopen the library once and type every entry point.  Raises if it is not built."""
    global _lib
    if _lib is not None:
        return _lib
    with _lock:
        if _lib is not None:
            return _lib
        if not os.path.exists(LIB_PATH):
            raise SeprLibraryError(
                f"{LIB_PATH} is missing: the HIP extension is not built. Run "
                "`python -c 'import __graft_entry__ as g; g.build()'` (or `make -C sepreformer_amd/csrc`). "
                "There is no CPU fallback for the separator path.")
        # torch bundles its own HIP runtime (torch/lib/libamdhip64.so).  It must be the one already in
        # the process when libsepr_hip.so is dlopen'ed, otherwise the loader binds this library to
        # /opt/rocm's copy and the two runtimes do not share devices or streams
        # ("no ROCm-capable device is detected" at the first launch).
        import torch  # noqa: F401
        lib = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(lib, name)  # AttributeError -> a declared symbol is not exported
            fn.restype = res
            fn.argtypes = args
        got = int(lib.sepr_version())
        if got != ABI_VERSION:      # the binding is derived from ONE header version: a stale .so would read short structs
            raise SeprLibraryError(f"{LIB_PATH} reports ABI {got}, this binding is written against include/sepr.h SEPR_VERSION {ABI_VERSION}: "
                                   "rebuild the library (`make -C sepreformer_amd/csrc`)")
        _lib = lib
        return lib


def check(rc: int, what: str) -> None:
    if rc == SEPR_OK:
        return
    msg = _ERR.get(rc, f"status {rc}")
    if rc == SEPR_EHIP:
        msg += ": " + load().sepr_last_hip_error().decode(errors="replace")
    raise RuntimeError(f"{what} failed: {msg}")


def version() -> int:
    return int(load().sepr_version())


def build_info() -> str:
    return load().sepr_build_info().decode()
