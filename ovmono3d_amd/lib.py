"""ctypes binding of libovm3d.so, derived from the C ABI declared in include/ovm3d.h.

The header is the only statement of the boundary: its constants, structs and prototypes are parsed once at import and published
here under their own names (``lib.OvmImage``, ``lib.OVM_SCENE_NOVEL``, ``lib.EXPORTS``). The parser is strict: a header line it
cannot turn into a layout or a signature is an error at import that names the line, never a silent skip.

The library is built in-tree by ``ovmono3d_amd/csrc/build.sh`` (``__graft_entry__.build()``).
There is no CPU or PyTorch fallback: if the shared object is missing or fails to load,
importing the native path raises.
"""
from __future__ import annotations

import ctypes as C
import math
import os
import re
from types import SimpleNamespace
from typing import Dict

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libovm3d.so")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "ovm3d.h")

_SCALARS = {"char": C.c_char, "int": C.c_int, "float": C.c_float, "double": C.c_double, "size_t": C.c_size_t,
            **{f"{u}int{b}_t": getattr(C, f"c_{u}int{b}") for u in ("", "u") for b in (8, 16, 32, 64)}}
_STARS = r"((?:\* ?(?:const ?)?)*)"         # the pointer part of a declarator, after whitespace is squeezed


class HeaderError(ValueError):
    """include/ovm3d.h holds something no layout or signature can be derived from."""


class StructPointer:
    """argtypes entry of a ``T*`` parameter, T a struct of the header. None, an integer and a c_void_p are addresses (device
    memory, a numpy buffer) and pass as they are; anything else must be what POINTER(T) takes: a T, byref(T), an array of T."""

    def __init__(self, struct):
        self.struct, self._typed = struct, C.POINTER(struct)

    def from_param(self, obj):
        if obj is None or isinstance(obj, (int, C.c_void_p)):
            return C.c_void_p.from_param(obj)
        return self._typed.from_param(obj)


def parse_header(text: str) -> SimpleNamespace:
    """C header text -> constants {name: int}, structs {name: ctypes.Structure} in declaration order, functions {name: (restype,
    argtypes)}. Takes what ovm3d.h is written in - integer #defines, anonymous enums, typedef'd structs of fixed-width scalars,
    pointers, arrays and earlier structs, opaque handles, prototypes - and raises HeaderError for anything else."""
    consts, structs, funcs, pointers = {}, {}, {}, {}
    types = dict(_SCALARS, void=None)       # None: incomplete (void, an opaque handle), usable behind a pointer only

    def fail(pos, msg):
        raise HeaderError(f"ovm3d.h:{text.count(chr(10), 0, pos) + 1}: {msg}")

    def blank(s):                           # keeps offsets, and so line numbers, valid
        return re.sub(r"[^\n]", " ", s)

    def ctype(pos, base, stars, param=False):
        if base not in types:
            fail(pos, f"unknown type {base!r}")
        if not stars:
            return types[base] if types[base] is not None else fail(pos, f"{base} used by value")
        if stars == 1 and base == "char":
            return C.c_char_p
        if stars == 1 and param and base in structs:
            return pointers.setdefault(base, StructPointer(structs[base]))
        return C.c_void_p

    def dim(pos, expr):                     # an integer, a constant, or sums of products of them
        try:
            return sum(math.prod(int(a) if a.strip().isdigit() else consts[a.strip()] for a in term.split("*")) for term in expr.split("+"))
        except KeyError:
            fail(pos, f"array dimension {expr!r} is not made of integers and known constants")

    def fields(pos, body):
        out = []
        for decl in filter(None, map(str.strip, body.split(";"))):
            m = re.fullmatch(r"(?:const )?(\w+) ?(.*)", decl) or fail(pos, f"cannot bind field {decl!r}")
            for d in m[2].split(","):
                dm = re.fullmatch(_STARS + r"(\w+)((?: ?\[[^\]]+\])*)", d.strip()) or fail(pos, f"cannot bind field {decl!r}")
                t = ctype(pos, m[1], dm[1].count("*"))
                for n in reversed(re.findall(r"\[([^\]]+)\]", dm[3])):      # leftmost dimension outermost
                    t = t * dim(pos, n)
                out.append((dm[2], t))
        return out

    def params(pos, args):
        out = []
        for a in [] if args.strip() == "void" else args.split(","):
            m = re.fullmatch(r"(?:const )?(\w+) ?" + _STARS + r"(\w+)", a.strip()) or fail(pos, f"cannot bind parameter {a.strip()!r}")
            out.append(ctype(pos, m[1], m[2].count("*"), param=True))
        return out

    def statement(pos, s):
        if m := re.fullmatch(r"typedef struct (\w+) \1", s):
            types[m[1]] = None
        elif m := re.fullmatch(r"typedef void ?\* ?(\w+)", s):
            types[m[1]] = C.c_void_p
        elif m := re.fullmatch(r"enum \{(.*)\}", s):
            value = -1
            for item in filter(None, map(str.strip, m[1].split(","))):
                e = re.fullmatch(r"(OVM_\w+)(?: ?= ?(-?\d+))?", item) or fail(pos, f"cannot bind enumerator {item!r}")
                consts[e[1]] = value = int(e[2]) if e[2] else value + 1
        elif m := re.fullmatch(r"typedef struct (\w+) ?\{(.*)\} ?\1", s):
            types[m[1]] = structs[m[1]] = type(m[1], (C.Structure,), {"_fields_": fields(pos, m[2]), "__module__": __name__})
        elif m := re.fullmatch(r"(const char ?\*|\w+) (ovm_\w+) ?\((.*)\)", s):
            if m[1] not in ("void", "int", "int32_t", "int64_t") and "*" not in m[1]:
                fail(pos, f"{m[2]}: return type {m[1]!r} is not int, int32_t, int64_t, const char* or void")
            funcs[m[2]] = (C.c_char_p if "*" in m[1] else types[m[1]], params(pos, m[3]))
        else:
            fail(pos, f"cannot bind {s[:80]!r}")

    text = re.sub(r"/\*.*?\*/|//[^\n]*", lambda m: blank(m[0]), text, flags=re.S)
    lines, pos, cxx = text.splitlines(keepends=True), 0, False
    for i, line in enumerate(lines):
        s = line.strip()
        if cxx or s.startswith("#"):        # directives; what only a C++ compiler sees (extern "C") is dropped
            if cxx:
                cxx = s != "#endif"
            elif m := re.fullmatch(r"# ?define (OVM_\w+) +(\(-?\d+\)|-?\d+)", s):
                consts[m[1]] = int(m[2].strip("()"))
            elif s == "#ifdef __cplusplus":
                cxx = True
            elif not re.fullmatch(r"#(include <\w+\.h>|ifndef OVM3D_H|define OVM3D_H|endif)", s):
                fail(pos, f"unsupported directive {s!r}")
            lines[i] = blank(line)
        pos += len(line)
    text = "".join(lines)

    depth = start = 0
    for m in re.finditer(r"[{};]", text):
        depth += {"{": 1, "}": -1, ";": 0}[m[0]]
        if m[0] == ";" and depth == 0:
            raw = text[start:m.start()]
            statement(start + len(raw) - len(raw.lstrip()), " ".join(raw.split()))
            start = m.end()
    if depth or text[start:].strip():
        fail(len(text) - len(text[start:].lstrip()), "declaration without an end")
    for what, pattern, bound in (("struct", r"typedef\s+struct\s+(\w+)\s*\{", structs), ("function", r"\b(ovm_\w+)\s*\(", funcs)):
        for m in re.finditer(pattern, text):
            if m[1] not in bound:
                fail(m.start(), f"{what} {m[1]} was not bound")
    return SimpleNamespace(constants=consts, structs=structs, functions=funcs)


with open(HEADER_PATH) as _f:
    _abi = parse_header(_f.read())
CONSTANTS, STRUCTS, FUNCTIONS = _abi.constants, _abi.structs, _abi.functions
globals().update(CONSTANTS)
globals().update(STRUCTS)
EXPORTS = list(FUNCTIONS)

# what the header cannot say: names for the profile categories and for the slots of OvmDecChainOp.lin[]
PROF_NAMES = ("attn", "qkv", "proj", "fc1", "fc2", "ln")
assert len(PROF_NAMES) == CONSTANTS["OVM_PROF_NCAT"]
STRUCTS["OvmDecChainOp"].LIN = ("ref0", "ref1", "sa_qk", "sa_v", "sa_out", "ca_q", "ca_out", "offw", "msda_out", "fc1", "fc2", "bb0", "bb1", "bb2")
assert len(STRUCTS["OvmDecChainOp"].LIN) == len(STRUCTS["OvmDecChainOp"]().lin)

_lib = None


def bind(cdll: C.CDLL, partial: bool = False) -> C.CDLL:
    """Give every function of the header its restype and argtypes on `cdll`. partial: a library built from an older header may
    lack some of them; otherwise a missing symbol raises."""
    for name, (restype, argtypes) in FUNCTIONS.items():
        if partial and not hasattr(cdll, name):
            continue
        fn = getattr(cdll, name)
        fn.restype, fn.argtypes = restype, argtypes
    return cdll


def load() -> C.CDLL:
    """Load libovm3d.so; raises (never falls back) when it is absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} not found: build it with ovmono3d_amd/csrc/build.sh (or __graft_entry__.build()). "
            "The native HIP path has no CPU fallback.")
    lib = bind(C.CDLL(LIB_PATH))
    for name, struct in STRUCTS.items():
        if lib.ovm_abi_sizeof(name.encode()) != C.sizeof(struct):
            raise RuntimeError(f"{LIB_PATH}: sizeof({name}) = {lib.ovm_abi_sizeof(name.encode())} but include/ovm3d.h gives "
                               f"{C.sizeof(struct)} bytes - rebuild the library (ovmono3d_amd/csrc/build.sh)")
    # experiment knobs, e.g. OVM_TUNE="gemm_bm=256,attn_tail=0"
    for kv in filter(None, os.environ.get("OVM_TUNE", "").split(",")):
        k, _, v = kv.partition("=")
        lib.ovm_tune_set(k.strip().encode(), int(v))
    _lib = lib
    return lib


class OvmError(RuntimeError):
    pass


def check(rc: int, handle=None, what: str = "") -> None:
    if rc == 0:
        return
    msg = ""
    if handle:
        msg = (load().ovm_last_error(handle) or b"").decode()
    raise OvmError(f"{what} failed with code {rc}: {msg}")


def make_tensor_table(state_dict: Dict[str, "np.ndarray"]):
    """state_dict values: contiguous float32 numpy arrays (host). Returns (ctypes array, keepalive)."""
    items = list(state_dict.items())
    arr = (STRUCTS["OvmTensor"] * len(items))()
    keep = []
    for i, (k, v) in enumerate(items):
        v = np.ascontiguousarray(v, dtype=np.float32)
        if v.ndim > 4:
            raise ValueError(f"{k}: more than 4 dims")
        kb = k.encode()
        keep.append((kb, v))
        arr[i].name = kb
        arr[i].data = v.ctypes.data
        arr[i].ndim = v.ndim
        for d in range(v.ndim):
            arr[i].shape[d] = v.shape[d]
    return arr, keep


def shard_range(n: int, rank: int, world: int):
    b, e = C.c_int64(), C.c_int64()
    check(load().ovm_host_shard_range(n, rank, world, C.byref(b), C.byref(e)), what="ovm_host_shard_range")
    return b.value, e.value


def interp_pos_embed(pos: "np.ndarray", G: int) -> "np.ndarray":
    """pos [1+M*M, D] float32 -> [1+G*G, D] (host, no GPU needed)."""
    pos = np.ascontiguousarray(pos, dtype=np.float32)
    M = int(round((pos.shape[0] - 1) ** 0.5))
    out = np.empty((1 + G * G, pos.shape[1]), dtype=np.float32)
    check(load().ovm_host_interp_pos_embed(pos.ctypes.data, M, pos.shape[1], G, out.ctypes.data),
          what="ovm_host_interp_pos_embed")
    return out
