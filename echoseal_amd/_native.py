"""ctypes binding of libechoseal_hip.so (C ABI: include/echoseal_hip.h).

There is deliberately NO fallback: if the shared library is missing or a call fails, an
exception is raised.  The hot path only ever runs on the HIP kernels.

The header is the one statement of the ABI: SIGNATURES and every ES_* constant of this module are read from it at import (bind_header).
"""
from __future__ import annotations

import ctypes
import os
import re
import sys

import torch  # noqa: F401  -- must be imported BEFORE the HIP library so that both share torch's HIP runtime
from ctypes import c_char_p, c_double, c_int, c_int64, c_uint32, c_void_p

_HERE = os.path.dirname(os.path.abspath(__file__))
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "echoseal_hip.h")


class NativeError(RuntimeError):
    pass


def variant_path(variant):
    """The library ES_LIB_VARIANT names: an A/B build made by tools/build_variant.sh or a mutant of tools/mutant_audit.py (same ABI check,
    same loud failure when missing).  The name goes into a file name, so it is letters, digits and underscores or it is refused."""
    if not variant:
        return os.path.join(_HERE, "libechoseal_hip.so")
    if not re.fullmatch(r"[A-Za-z0-9_]+", variant):
        raise NativeError(f"ES_LIB_VARIANT={variant!r} is not a variant name ([A-Za-z0-9_]+)")
    return os.path.join(_HERE, f"libechoseal_hip_{variant}.so")


LIB_VARIANT = os.environ.get("ES_LIB_VARIANT", "")
LIB_PATH = variant_path(LIB_VARIANT)

# The binding rule.  A parameter: a pointer is c_void_p -- except `const char*` and a `const uint8_t* <name>_host` (bytes objects: c_char_p);
# a scalar is one of the four below.  A return type is one of _RESTYPES.  Anything else is refused by name.
_SCALARS = {"int": c_int, "int64_t": c_int64, "uint32_t": c_uint32, "double": c_double}
_RESTYPES = {"int": c_int, "void": None, "es_ctx*": c_void_p, "const char*": c_char_p}
_INT = r"(?:0[xX][0-9a-fA-F]+|[0-9]+)[uUlL]*"


def _ctype(name, ctype, param):
    if ctype in _SCALARS:
        return _SCALARS[ctype]
    if re.fullmatch(r"(?:const )?\w+\*", ctype):
        return c_char_p if ctype == "const char*" or (ctype == "const uint8_t*" and param.endswith("_host")) else c_void_p
    raise NativeError(f"{name}: parameter `{ctype} {param}` has a type outside the binding rule (_native.bind_header)")


def _define(name, value):
    """An integer literal (decimal or hex, u / l suffixes, a sign, parentheses) or `a << b` of two of them."""
    v = value.strip()
    while v.startswith("(") and v.endswith(")"):
        v = v[1:-1].strip()
    m = re.fullmatch(rf"(-?{_INT})(?:\s*<<\s*({_INT}))?", v)
    if not m:
        raise NativeError(f"#define {name} {value.strip()}: not an integer literal or `a << b` (_native.bind_header)")
    a, b = (int(g.rstrip("uUlL"), 0) if g else 0 for g in m.groups())
    return a << b


def bind_header(text):
    """(declarations, signatures, constants) of a header in the style of include/echoseal_hip.h: name -> [(C type, parameter name)],
    name -> (restype, argtypes), ES_* name -> int.  Nothing is skipped: a type or a value outside the rule raises NativeError."""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    constants = {name: _define(name, value) for name, value in re.findall(r"^[ \t]*#[ \t]*define[ \t]+(ES_\w+)[ \t]+(.*?)[ \t]*$", text, re.M)}
    text = re.sub(r"^[ \t]*#.*$", " ", text, flags=re.M)
    declarations, signatures = {}, {}
    for ret, name, params in re.findall(r"([\w \t*]+?)\b(es_\w+)\s*\(([^()]*)\)\s*;", text):
        ret = re.sub(r"\s*\*", "*", " ".join(ret.split()))
        if ret not in _RESTYPES:
            raise NativeError(f"{name}: return type `{ret}` is outside the binding rule (_native.bind_header)")
        decl = []
        for p in ([] if params.strip() in ("", "void") else params.split(",")):
            m = re.fullmatch(r"(.*?)(\w+)", " ".join(p.split()))
            if not m or not m.group(1).strip():
                raise NativeError(f"{name}: cannot read the parameter `{p.strip()}` (_native.bind_header)")
            decl.append((re.sub(r"\s*\*", "*", m.group(1).strip()), m.group(2)))
        declarations[name] = decl
        signatures[name] = (_RESTYPES[ret], [_ctype(name, t, n) for t, n in decl])
    return declarations, signatures, constants


try:
    with open(HEADER_PATH) as _f:
        DECLARATIONS, SIGNATURES, CONSTANTS = bind_header(_f.read())
except OSError as e:
    raise NativeError(f"{HEADER_PATH}: the C ABI's header is what this module binds from ({e})") from None
globals().update(CONSTANTS)              # ES_ABI_VERSION (load() refuses a library built from another one), ES_FRAME_LEN, ES_DTYPE_F32 ...

# The companion header of the presence test, bound by the same rule into tables of its own: the three above stay the statement
# of include/echoseal_hip.h alone.  load() sets these argtypes too, and RxEngine._call finds the names on the library like any other.
PRESENCE_HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "echoseal_presence.h")
try:
    with open(PRESENCE_HEADER_PATH) as _f:
        PRESENCE_DECLARATIONS, PRESENCE_SIGNATURES, PRESENCE_CONSTANTS = bind_header(_f.read())
except OSError as e:
    raise NativeError(f"{PRESENCE_HEADER_PATH}: the presence calls are bound from this header ({e})") from None
if set(PRESENCE_SIGNATURES) & set(SIGNATURES) or set(PRESENCE_CONSTANTS) & set(CONSTANTS):
    raise NativeError(f"{PRESENCE_HEADER_PATH} declares a name include/echoseal_hip.h already has")
globals().update(PRESENCE_CONSTANTS)     # ES_HOP_TILE, ES_HOP_ORIGINS

# The companion header of the drift-following presence test, bound the same way into three more tables.
WARP_HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "echoseal_warp.h")
try:
    with open(WARP_HEADER_PATH) as _f:
        WARP_DECLARATIONS, WARP_SIGNATURES, WARP_CONSTANTS = bind_header(_f.read())
except OSError as e:
    raise NativeError(f"{WARP_HEADER_PATH}: the warp calls are bound from this header ({e})") from None
if set(WARP_SIGNATURES) & (set(SIGNATURES) | set(PRESENCE_SIGNATURES)) or set(WARP_CONSTANTS) & (set(CONSTANTS) | set(PRESENCE_CONSTANTS)):
    raise NativeError(f"{WARP_HEADER_PATH} declares a name another header already has")
globals().update(WARP_CONSTANTS)         # ES_WARP_HB

# The companion header of the presence test over records anywhere in a table of rows, bound the same way into three more tables.
LIVE_PRESENCE_HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "echoseal_live_presence.h")
try:
    with open(LIVE_PRESENCE_HEADER_PATH) as _f:
        LIVE_PRESENCE_DECLARATIONS, LIVE_PRESENCE_SIGNATURES, LIVE_PRESENCE_CONSTANTS = bind_header(_f.read())
except OSError as e:
    raise NativeError(f"{LIVE_PRESENCE_HEADER_PATH}: the live presence calls are bound from this header ({e})") from None
if (set(LIVE_PRESENCE_SIGNATURES) & (set(SIGNATURES) | set(PRESENCE_SIGNATURES) | set(WARP_SIGNATURES))
        or set(LIVE_PRESENCE_CONSTANTS) & (set(CONSTANTS) | set(PRESENCE_CONSTANTS) | set(WARP_CONSTANTS))):
    raise NativeError(f"{LIVE_PRESENCE_HEADER_PATH} declares a name another header already has")
globals().update(LIVE_PRESENCE_CONSTANTS)

# The companion header of the hypothesis list picked on the device, bound the same way into three more tables.
PICK_HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "echoseal_pick.h")
try:
    with open(PICK_HEADER_PATH) as _f:
        PICK_DECLARATIONS, PICK_SIGNATURES, PICK_CONSTANTS = bind_header(_f.read())
except OSError as e:
    raise NativeError(f"{PICK_HEADER_PATH}: the device pick is bound from this header ({e})") from None
if (set(PICK_SIGNATURES) & (set(SIGNATURES) | set(PRESENCE_SIGNATURES) | set(WARP_SIGNATURES) | set(LIVE_PRESENCE_SIGNATURES))
        or set(PICK_CONSTANTS) & (set(CONSTANTS) | set(PRESENCE_CONSTANTS) | set(WARP_CONSTANTS) | set(LIVE_PRESENCE_CONSTANTS))):
    raise NativeError(f"{PICK_HEADER_PATH} declares a name another header already has")
globals().update(PICK_CONSTANTS)         # ES_PICK_MAX_H

# The companion header of the coherent presence test, bound the same way into three more tables.
COHERENT_HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "echoseal_coherent.h")
try:
    with open(COHERENT_HEADER_PATH) as _f:
        COHERENT_DECLARATIONS, COHERENT_SIGNATURES, COHERENT_CONSTANTS = bind_header(_f.read())
except OSError as e:
    raise NativeError(f"{COHERENT_HEADER_PATH}: the coherent presence calls are bound from this header ({e})") from None
if (set(COHERENT_SIGNATURES) & (set(SIGNATURES) | set(PRESENCE_SIGNATURES) | set(WARP_SIGNATURES) | set(LIVE_PRESENCE_SIGNATURES) | set(PICK_SIGNATURES))
        or set(COHERENT_CONSTANTS) & (set(CONSTANTS) | set(PRESENCE_CONSTANTS) | set(WARP_CONSTANTS) | set(LIVE_PRESENCE_CONSTANTS) | set(PICK_CONSTANTS))):
    raise NativeError(f"{COHERENT_HEADER_PATH} declares a name another header already has")
globals().update(COHERENT_CONSTANTS)     # ES_MF_TILE, ES_COH_TILE, ES_COH_HDR_PN

# The companion header of the coherent score over records anywhere in a table of rows, bound the same way into three more tables.
COHERENT_AT_HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "echoseal_coherent_at.h")
try:
    with open(COHERENT_AT_HEADER_PATH) as _f:
        COHERENT_AT_DECLARATIONS, COHERENT_AT_SIGNATURES, COHERENT_AT_CONSTANTS = bind_header(_f.read())
except OSError as e:
    raise NativeError(f"{COHERENT_AT_HEADER_PATH}: the coherent score over records is bound from this header ({e})") from None
if (set(COHERENT_AT_SIGNATURES) & (set(SIGNATURES) | set(PRESENCE_SIGNATURES) | set(WARP_SIGNATURES) | set(LIVE_PRESENCE_SIGNATURES) | set(PICK_SIGNATURES)
                                   | set(COHERENT_SIGNATURES))
        or set(COHERENT_AT_CONSTANTS) & (set(CONSTANTS) | set(PRESENCE_CONSTANTS) | set(WARP_CONSTANTS) | set(LIVE_PRESENCE_CONSTANTS) | set(PICK_CONSTANTS)
                                         | set(COHERENT_CONSTANTS))):
    raise NativeError(f"{COHERENT_AT_HEADER_PATH} declares a name another header already has")
globals().update(COHERENT_AT_CONSTANTS)  # none so far

_lib = None


def load() -> ctypes.CDLL:
    """Load the HIP library (once).  Raises if it has not been built -- never falls back."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise NativeError(
            f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "or `make -C echoseal_amd/csrc`.  There is no CPU fallback for the EchoSeal hot path.")
    lib = ctypes.CDLL(LIB_PATH)
    try:
        lib.es_abi_version.restype = c_int
        got = int(lib.es_abi_version())
    except AttributeError:
        got = None
    if got != CONSTANTS["ES_ABI_VERSION"]:
        raise NativeError(f"{LIB_PATH} reports ABI version {got}, this package binds version {CONSTANTS['ES_ABI_VERSION']} "
                          "(table strides and signatures differ between versions): rebuild it with `make -C echoseal_amd/csrc`")
    for name, (res, args) in {**SIGNATURES, **PRESENCE_SIGNATURES, **WARP_SIGNATURES, **LIVE_PRESENCE_SIGNATURES, **PICK_SIGNATURES,
                             **COHERENT_SIGNATURES, **COHERENT_AT_SIGNATURES}.items():
        fn = getattr(lib, name)          # AttributeError here means header and library disagree
        fn.restype = res
        fn.argtypes = args
    if LIB_VARIANT:                      # said once: load() returns the cached library from here on
        print(f"echoseal_amd: loaded variant library {os.path.basename(LIB_PATH)} (ES_LIB_VARIANT={LIB_VARIANT})", file=sys.stderr)
    _lib = lib
    return lib


def check(ctx, rc: int, what: str) -> None:
    if rc != 0:
        msg = load().es_last_error(ctx)
        raise NativeError(f"{what} failed (code {rc}): {msg.decode() if msg else '?'}")
