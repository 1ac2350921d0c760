"""ctypes binding of libpytc_hip.so, derived from include/pytc_hip.h.

The header is the one declaration of the C ABI: its prototypes, argument structs and ``PYTC_*`` codes are read at import by
``parse_header`` and become the ``argtypes`` / ``restype`` of every entry point, the ``ctypes.Structure`` classes and this
module's constants.  Nothing of the ABI is restated here, so adding an entry point means writing the kernel, its prototype
and its wrapper in hip_ops.py.

There is deliberately NO fallback: if the library is missing or a call fails, a RuntimeError
is raised.  The library is built in-tree by ``python -m pytorch_connectomics_amd.csrc.build``
(also run by ``__graft_entry__.build()``).
"""
from __future__ import annotations

import ctypes as C
import os
import re
from pathlib import Path

LIB_PATH = Path(__file__).resolve().parent / "lib" / "libpytc_hip.so"
HEADER_PATH = Path(__file__).resolve().parent.parent / "include" / "pytc_hip.h"

_SCALARS = {"int": C.c_int, "int32_t": C.c_int32, "int64_t": C.c_int64, "float": C.c_float, "double": C.c_double}
_RETURNS = {"int": C.c_int, "int64_t": C.c_int64, "const char*": C.c_char_p}


def parse_header(text: str):
    """include/pytc_hip.h -> (constants {NAME: int}, structs {C name: Structure class}, signatures {name: (restype, argtypes)}).

    Reads this header, not C in general: whatever is not an integer ``#define PYTC_<NAME>``, a ``typedef struct {...} pytc_<name>;``
    of scalars, pointers and fixed arrays, or a ``<ret> pytc_<name>(<params>);`` prototype raises a ValueError that names it."""
    def fail(what):
        raise ValueError(f"pytc_hip.h: {what}")

    text = re.sub(r"//[^\n]*", " ", re.sub(r"/\*.*?\*/", " ", text, flags=re.S))
    constants, structs, signatures = {}, {}, {}
    for line in re.findall(r"^[ \t]*#[^\n]*", text, flags=re.M):
        m = re.match(r"\s*#\s*define\s+PYTC_(\w+)(.*)", line)
        if m and m.group(1) != "HIP_H":
            try:
                constants[m.group(1)] = int(m.group(2), 0)
            except ValueError:
                fail(f"#define PYTC_{m.group(1)} is not an integer literal: {m.group(2).strip()!r}")
    code = re.sub(r"^[ \t]*#[^\n]*", " ", text, flags=re.M)
    code, wrapped = re.subn(r'extern\s+"C"\s*\{', " ", code)
    if wrapped:
        code = re.sub(r"\}\s*$", " ", code)

    def scalar(ctype, where):
        if ctype in structs:
            fail(f"{where}: struct {ctype} by value")
        if ctype not in _SCALARS:
            fail(f"{where}: unknown type {ctype!r}")
        return _SCALARS[ctype]

    def struct(m):
        fields = []
        for decl in filter(None, (" ".join(d.split()) for d in m.group(1).split(";"))):
            where = f"{m.group(2)}: field {decl!r}"
            if "*" in decl:
                ptr = re.fullmatch(r"[\w ]+\*[ *]*(?:const )?(\w+)", decl) or fail(f"{where} is unreadable")
                fields.append((ptr.group(1), C.c_void_p))
                continue
            ctype, _, names = re.sub(r"^const ", "", decl).partition(" ")
            for name in names.split(","):
                d = re.fullmatch(r" ?(\w+) ?(?:\[ ?(\w+) ?\])? ?", name) or fail(f"{where} is unreadable")
                ftype, bound = scalar(ctype, where), d.group(2)
                if bound is not None:
                    n = int(bound) if bound.isdigit() else constants.get(bound[5:] if bound.startswith("PYTC_") else None)
                    if n is None:
                        fail(f"{where}: array bound {bound!r} is neither an integer literal nor a PYTC_ define")
                    ftype = ftype * n
                fields.append((d.group(1), ftype))
        structs[m.group(2)] = type(m.group(2), (C.Structure,), {"_fields_": fields})
        return " "

    code = re.sub(r"typedef\s+struct\s*\w*\s*\{([^{}]*)\}\s*(pytc_\w+)\s*;", struct, code)

    def param(p, proto):
        where = f"{proto}: parameter {p!r}"
        if "*" in p:
            # the pointee, then every "*" (a "* const" counts as one), then the optional name
            m = re.fullmatch(r"(?:const )?(\w+) ?(\*[ *]*)(\w+)?", re.sub(r" ?\* ?const\b", "*", p)) or fail(f"{where} is unreadable")
            pointee = m.group(1) if m.group(2).count("*") == 1 else None
            return C.POINTER(structs[pointee]) if pointee in structs else C.c_char_p if pointee == "char" else C.c_void_p
        m = re.fullmatch(r"(?:const )?(\w+)(?: \w+)?", p) or fail(f"{where} is unreadable")
        return scalar(m.group(1), where)

    for stmt in filter(None, (" ".join(s.split()) for s in code.split(";"))):
        m = re.fullmatch(r"(int|int64_t|const char ?\*) ?(pytc_\w+) ?\((.*)\)", stmt) or fail(f"unreadable declaration {stmt!r}")
        ret, name, params = m.group(1).replace(" *", "*"), m.group(2), m.group(3).strip()
        if name in signatures:
            fail(f"{name} is declared twice")
        if "(" in params or "..." in params:
            fail(f"{name}: function pointers and variadic parameters are not supported: {params!r}")
        signatures[name] = (_RETURNS[ret], [] if params == "void" else [param(p.strip(), name) for p in params.split(",")])
    stragglers = set(re.findall(r"\b(pytc_\w+)\s*\(", text)) ^ set(signatures)
    if stragglers:
        fail(f"not parsed as prototypes: {sorted(stragglers)}")
    return constants, structs, signatures


if not HEADER_PATH.exists():
    raise RuntimeError(f"pytorch_connectomics_amd: the C ABI declaration {HEADER_PATH} is missing; the binding is derived from it")
CONSTANTS, STRUCTS, SIGNATURES = parse_header(HEADER_PATH.read_text())

# every `#define PYTC_<NAME> <integer>` of include/pytc_hip.h, without the prefix: OK, ERR_INVALID, ABI_VERSION, F32, BF16, ACT_GELU,
# RES_NORM_BWD, VIEW_FLIP_Z, LABEL_AFFINITY, ... -- grep the header for a name that is not assigned in this file
globals().update(CONSTANTS)
# the argument structs under the class names their callers use
globals().update({py_name: STRUCTS[c_name] for c_name, py_name in {
    "pytc_pw_args": "PwArgs", "pytc_mlp_args": "MlpArgs", "pytc_conv3d_args": "Conv3dArgs", "pytc_reduce_item": "ReduceItem",
    "pytc_label_channel": "LabelChannel"}.items()})

# user-facing names -> header codes (an entry whose define is renamed or removed fails here, at import)
# (noqa F821: a linter cannot see the names the update above defines)
VIEW_SWAPS = {VIEW_SWAP_YX: (1, 2), VIEW_SWAP_ZY: (0, 1), VIEW_SWAP_ZX: (0, 2)}      # noqa: F821 -- swap bit -> the two window axes it exchanges
PAD_MODES = {"constant": PAD_CONSTANT, "reflect": PAD_REFLECT, "replicate": PAD_REPLICATE, "circular": PAD_CIRCULAR}  # noqa: F821
RAW_DTYPES = {"uint8": RAW_U8, "int8": RAW_I8, "uint16": RAW_U16, "int16": RAW_I16,  # noqa: F821
              "uint32": RAW_U32, "int32": RAW_I32, "float32": RAW_F32, "float64": RAW_F64}  # noqa: F821
LABEL_EDGE_MODES = {"all": LABEL_EDGE_ALL, "seg-all": LABEL_EDGE_SEG_ALL, "seg-no-bg": LABEL_EDGE_SEG_NO_BG}  # noqa: F821
LABEL_MAX_EROSION = 10      # the largest border half-width pytc_seg_erode_instance accepts per axis

_lib = None


def exported_symbols():
    """Names every build of the library must export (checked by the CPU test-suite)."""
    return sorted(SIGNATURES)


def lib():
    """Load (once) and return the ctypes handle; raise loudly if it is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not LIB_PATH.exists():
        raise RuntimeError(
            f"pytorch_connectomics_amd: HIP library {LIB_PATH} is missing. Build it with "
            "`python -m pytorch_connectomics_amd.csrc.build` (needs hipcc). There is no CPU fallback.")
    # torch first: it ships its own libamdhip64 -- loaded before ours, the library's HIP symbols bind to the runtime
    # PyTorch's tensors and streams live in; loaded after, the process ends up with two HIP runtimes and this library
    # sees no device
    import torch  # noqa: F401
    handle = C.CDLL(str(LIB_PATH))
    for name, (res, args) in SIGNATURES.items():
        try:
            fn = getattr(handle, name)
        except AttributeError as e:  # pragma: no cover
            raise RuntimeError(f"{LIB_PATH} does not export {name}; rebuild the library") from e
        fn.restype = res
        fn.argtypes = args
    if handle.pytc_abi_version() != ABI_VERSION:  # noqa: F821
        raise RuntimeError(f"libpytc_hip.so ABI version {handle.pytc_abi_version()} != {ABI_VERSION} "  # noqa: F821
                           "(include/pytc_hip.h PYTC_ABI_VERSION); rebuild the library")
    _lib = handle
    # PYTC_TUNING="knob=value,knob=value": kernel-variant knobs (pytc_set_tuning) for A/B runs of unmodified commands
    for item in filter(None, (t.strip() for t in os.environ.get("PYTC_TUNING", "").split(","))):
        key, sep, val = item.partition("=")
        try:
            ok = bool(sep) and bool(key.strip()) and handle.pytc_set_tuning(key.strip().encode(), int(val)) == OK  # noqa: F821
        except ValueError:
            ok = False
        if not ok:
            raise RuntimeError(f"PYTC_TUNING: cannot set {item!r} (expected knob=integer[,knob=integer...])")
    return _lib


def check(status: int, what: str) -> None:
    if status != OK:  # noqa: F821
        msg = lib().pytc_last_error()
        raise RuntimeError(f"{what} failed (status {status}): {msg.decode() if msg else '?'}")
