"""ctypes binding of lib/libsmml_hip.so (C-ABI declared in include/smml.h).

The product path has no CPU or eager fallback: if the library is missing, or a tensor is not a
contiguous fp32 CUDA(HIP) tensor, the call fails loudly."""
from __future__ import annotations

import ctypes as C
import os
import re
from typing import Optional

import torch

_PKG = os.path.dirname(os.path.abspath(__file__))
# SMML_LIB: measurement hook - load another build of the same C-ABI (tests/tools/build_variants.py writes them to lib/variants/)
LIB_PATH = os.environ.get("SMML_LIB") or os.path.join(_PKG, "lib", "libsmml_hip.so")

HEADER_PATH = os.path.join(os.path.dirname(_PKG), "include", "smml.h")


class DeformOpts(C.Structure):
    """SmmlDeformOpts of include/smml.h: optional behaviour of ONE fused deformable-attention launch, passed with the call.
    _fields_ are the header's, set below."""


_SCALARS = {"int": C.c_int, "long long": C.c_longlong, "unsigned long long": C.c_ulonglong, "float": C.c_float, "size_t": C.c_size_t}


def _ctype(ctext: str, where: str, ret: bool = False):
    """ctypes type of a C type as include/smml.h writes it: device and host pointers travel as void*, scalars by the table above."""
    t = " ".join(ctext.replace("*", " * ").split())
    if t == "void" and ret:
        return None
    if t == "const char *" and ret:
        return C.c_char_p
    if t == "const SmmlDeformOpts *":
        return C.POINTER(DeformOpts)
    if re.fullmatch(r"(const )?\w+( \w+)* \*", t):
        return C.c_void_p
    if t not in _SCALARS:
        raise RuntimeError(f"include/smml.h: type `{ctext.strip()}` of `{where}` is not one the ctypes binding knows")
    return _SCALARS[t]


def _declarator(text: str, where: str):
    """`type name` -> (name, ctypes type, the type is `float*` / `const float*`)"""
    m = re.fullmatch(r"\s*([\w\s]*[\w*])\s*\b([A-Za-z_]\w*)\s*", text)
    if not m or m.group(2) in ("int", "long", "float", "void", "unsigned", "size_t", "char", "short", "const"):
        raise RuntimeError(f"include/smml.h: cannot read `{text.strip()}` of `{where}` as `type name`")
    return m.group(2), _ctype(m.group(1), where), re.sub(r"\bconst\b|\s", "", m.group(1)) == "float*"


def parse_prototypes(text: str, params: Optional[dict] = None) -> dict:
    """name -> (restype, [argtypes]) for C text that holds prototypes `ret smml_name(type name, ...);` and nothing else besides
    comments, preprocessor lines and the extern "C" bracket.  Strict: whatever it cannot read raises, with the offending text.
    params (a dict) receives name -> [(parameter name, ctypes type, pointee is float)]: what `bind` calls an entry point by."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    text = re.sub(r"^[ \t]*#.*$", " ", text, flags=re.M)
    text = re.sub(r'extern\s+"C"\s*\{(.*)\}', r"\1", text, flags=re.S)
    sigs = {}
    *protos, tail = text.split(";")
    if tail.strip():
        raise RuntimeError(f"include/smml.h: `{' '.join(tail.split())}` does not end in `;`")
    for proto in protos:
        m = re.fullmatch(r"\s*([\w\s*]+?)\b(smml_\w+)\s*\(([^()]*)\)\s*", proto)
        if not m or m.group(2) in sigs:
            raise RuntimeError(f"include/smml.h: cannot read `{' '.join(proto.split())}` as one prototype `ret smml_name(type name, ...)`")
        ret, name, plist = m.groups()
        decl = [] if plist.strip() == "void" else [_declarator(p, name) for p in plist.split(",")]
        sigs[name] = (_ctype(ret, name, ret=True), [t for _, t, _ in decl])
        if params is not None:
            params[name] = decl
    return sigs


def parse_header(text: str, params: Optional[dict] = None):
    """(SMML_ABI_VERSION, the fields of SmmlDeformOpts, name -> (restype, [argtypes])) of the text of include/smml.h; params: as in
    parse_prototypes"""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    abi = re.search(r"^[ \t]*#[ \t]*define[ \t]+SMML_ABI_VERSION[ \t]+(\d+)[ \t]*$", text, re.M)
    struct = re.search(r"typedef\s+struct\s+SmmlDeformOpts\s*\{(.*?)\}\s*SmmlDeformOpts\s*;", text, re.S)
    if not abi or not struct:
        raise RuntimeError("include/smml.h: SMML_ABI_VERSION or struct SmmlDeformOpts not found")
    fields = [_declarator(f, "SmmlDeformOpts")[:2] for f in struct.group(1).split(";") if f.strip()]
    return int(abi.group(1)), fields, parse_prototypes(text[:struct.start()] + text[struct.end():], params)


if not os.path.exists(HEADER_PATH):
    raise RuntimeError(f"{HEADER_PATH} is missing: the ctypes binding is derived from it (it ships with the repository, next to the package)")
# ABI_VERSION: smml_abi_version() of the library this binding is for; SIGNATURES: name -> (restype, argtypes), as the header declares them;
# PARAMS: name -> [(parameter name, ctypes type, pointee is float)] - the header's parameter names are binding: `bind` calls by them
PARAMS: dict = {}
with open(HEADER_PATH) as _h:
    ABI_VERSION, DeformOpts._fields_, SIGNATURES = parse_header(_h.read(), PARAMS)

_lib: Optional[C.CDLL] = None


def lib() -> C.CDLL:
    """Loads the shared library once; raises if it has not been built (no fallback)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(hipcc --offload-arch=gfx950); there is no CPU or eager fallback for this path")
        handle = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(handle, name)      # AttributeError if the symbol is not exported
            fn.restype = res
            fn.argtypes = args
        if handle.smml_abi_version() != ABI_VERSION:
            raise RuntimeError(f"{LIB_PATH} implements C-ABI version {handle.smml_abi_version()}, this package binds version {ABI_VERSION}: rebuild it")
        if os.environ.get("SMML_GEMM_MODE"):       # measurement switch: 1 = fp32-MFMA GEMM only, 2 = split-bf16 wherever it applies
            handle.smml_gemm_set_mode(int(os.environ["SMML_GEMM_MODE"]))
        if os.environ.get("SMML_GEMM_SMALL_TILE"):  # measurement switch: 1 = never the 64-row tile, 2 = wherever it applies
            handle.smml_gemm_set_small_tile(int(os.environ["SMML_GEMM_SMALL_TILE"]))
        _lib = handle
    return _lib


def deform_opts(seed_offset: Optional[torch.Tensor] = None, log_distance: bool = True, mask_table: Optional[torch.Tensor] = None,
                mask_table_pmax: float = 0.0, export_masks: Optional[torch.Tensor] = None, region_lds_cap: int = 0):
    """The `opts` argument of a fused deformable-attention entry point (byref of a DeformOpts), or None when every field is at its default.
    The struct is read during the call only; the tensors it points at must outlive the launch (the callers keep them)."""
    if seed_offset is None and log_distance and mask_table is None and export_masks is None and not region_lds_cap:
        return None
    if seed_offset is not None and (seed_offset.dtype != torch.int64 or seed_offset.numel() != 1):
        raise RuntimeError("dropout_seed_offset must be a device int64 tensor with one element")
    o = DeformOpts(ptr(seed_offset), 0 if log_distance else 1, ptr(mask_table), float(mask_table_pmax), ptr(export_masks), int(region_lds_cap))
    return C.byref(o)


def check(rc: int, what: str = "") -> None:
    if rc != 0:
        msg = lib().smml_last_error().decode("utf-8", "replace")
        raise RuntimeError(f"smml call failed ({rc}){': ' + what if what else ''}: {msg}")


def ptr(t: Optional[torch.Tensor]):
    """Raw device pointer of a contiguous fp32/int32/uint8 HIP tensor (None -> NULL)."""
    if t is None:
        return None
    if not t.is_cuda:
        raise RuntimeError("smml kernels need tensors resident in GPU HBM (got a CPU tensor); "
                           "this path has no CPU fallback")
    if not t.is_contiguous():
        raise RuntimeError("smml kernels need contiguous tensors")
    if t.device.index != torch.cuda.current_device():
        # the C entry points launch on the current HIP device and stream() hands them that device's stream: a tensor of another
        # device would be dereferenced by a kernel running elsewhere (one process per GPU: torch.cuda.set_device(LOCAL_RANK))
        raise RuntimeError(f"smml kernels launch on the current device (cuda:{torch.cuda.current_device()}) but got a tensor on "
                           f"{t.device}; call torch.cuda.set_device first (one process per GPU)")
    return C.c_void_p(t.data_ptr())


def fptr(t: Optional[torch.Tensor]):
    if t is not None and t.dtype != torch.float32:
        raise RuntimeError(f"smml fp32 kernel got dtype {t.dtype}")
    return ptr(t)


def stream(device=None):
    """The current HIP stream of `device` (default: the current device) as a void*."""
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def _plan(decl):
    """[(parameter name, what turns a tensor into that argument)] of one prototype's PARAMS row: fptr for a `float*` (the fp32 check),
    ptr for any other pointer"""
    return [(pname, fptr if is_float else ptr if ctype is C.c_void_p else None) for pname, ctype, is_float in decl]


_PLANS = {name: _plan(decl) for name, decl in PARAMS.items()}     # resolved once: a launch costs one lookup per parameter


def bind(name: str, values, params: Optional[dict] = None) -> list:
    """The arguments of the entry point `name` in its prototype's order, each taken from the mapping `values` by its parameter name
    (`values` may hold more: one namespace serves every entry point of a family).  Tensors become device pointers - fptr for a
    `float*` parameter, ptr for any other pointer; None is NULL; scalars and ready-made c_void_p / byref values pass unchanged.
    params: prototypes other than the header's (parse_prototypes; tests)."""
    out = []
    for pname, conv in _PLANS[name] if params is None else _plan(params[name]):
        try:
            v = values[pname]
        except KeyError:
            raise RuntimeError(f"{name}: no value for its parameter `{pname}`") from None
        out.append(conv(v) if conv is not None and isinstance(v, torch.Tensor) else v)
    return out


def call(name: str, values, keys=None):
    """What the entry point `name` returns for the arguments `bind` takes from `values` (a status for check(), or a size).  keys: the
    key set the caller states for this namespace (a constant a test can hold against the header); `values` must hold exactly those."""
    if keys is not None and values.keys() != keys:
        raise RuntimeError(f"{name}: the namespace holds {sorted(values)}, its key set names {sorted(keys)}")
    return getattr(lib(), name)(*bind(name, values))
