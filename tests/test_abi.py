"""The C-ABI library loads and exports every symbol include/ovm3d.h declares (no GPU compute calls)."""
import ctypes as C
import os
import re

import pytest

from common import ROOT


def _declared():
    txt = open(os.path.join(ROOT, "include", "ovm3d.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(ovm_[a-z0-9_]+)\s*\(", txt)))


def test_exports_every_declared_symbol():
    from ovmono3d_amd import lib
    L = lib.load()
    names = _declared()
    assert len(names) >= 20
    for n in names:
        assert hasattr(L, n), f"libovm3d.so does not export {n}"
    assert sorted(lib.EXPORTS) == names, "lib.EXPORTS out of sync with include/ovm3d.h"


def test_struct_layouts_match_header():
    from ovmono3d_amd import lib
    # OvmDet3D is 48 x 4 bytes; OvmImage / OvmTensor as declared
    assert lib.OVM_REC_FLOATS * 4 == 192
    assert C.sizeof(lib.OvmImage) == 8 + 4 + 4 + 8 * 3 + 4 + 4 + 36 + 4          # trailing pad to 8
    assert C.sizeof(lib.OvmTensor) == 8 + 8 + 8 + 32
    assert C.sizeof(lib.OvmConfig) == 4 * 7 + 12 + 12 + 4 * 5 + 4 + 16 + 12 + 4 * 2 + 4 + 4 + 4 + 4 + 4 * 3 + 4 * 3
    assert C.sizeof(lib.OvmGemmEpiOp) == 4 * 12 + 8 * 6 + 4 * 2 + 8 + 4 * 2 + 8 + 8 + 4 * 2 + 8 * 2 + 4 * 4 + 8 * 3 + 4 * 4 + 8 + 4 * 4
    assert C.sizeof(lib.OvmAttnF32Op) == 8 * 3 + 4 * 4 + 8 * 6 + (8 + 4 * 2 + 8 * 2) + (8 * 2 + 4 * 2 + 8 * 2) + 4 * 6 + (8 + 8 + 4 * 2) * 2 + 8 * 2 + 4 * 2
    assert C.sizeof(lib.OvmMsDeformOp) == 8 * 3 + 4 * 4 + 4 * 6 + 4 * 24 + 8 * 3 + 4 * 2
    assert C.sizeof(lib.OvmRowOp) == 8 * 6 + 4 * 8 + 4 * 2 + 8 * 6 + 4 * 6
    # and the library agrees with every mirror (lib.load() also refuses a mismatch)
    L = lib.load()
    for name, mirror in (("OvmConfig", lib.OvmConfig), ("OvmTensor", lib.OvmTensor), ("OvmImage", lib.OvmImage),
                         ("OvmGdinoConfig", lib.OvmGdinoConfig), ("OvmGemmEpiOp", lib.OvmGemmEpiOp)):
        assert L.ovm_abi_sizeof(name.encode()) == C.sizeof(mirror), name
    for name, mirror in (("OvmAttnF32Op", lib.OvmAttnF32Op), ("OvmMsDeformOp", lib.OvmMsDeformOp), ("OvmRowOp", lib.OvmRowOp)):
        assert L.ovm_abi_sizeof(name.encode()) == C.sizeof(mirror), name
    assert L.ovm_abi_sizeof(b"OvmDecChainOp") == C.sizeof(lib.OvmDecChainOp) == 4 * 6 + 8 * 8 + (8 * 3 + 4 * 2) + 4 * 26 + 32 * 14 + 16 * 4 + (4 * 2 + 8 * 2)
    assert L.ovm_abi_sizeof(b"OvmDet3D") == 192 and L.ovm_abi_sizeof(b"nope") == -1


def test_parsed_layouts_match_a_c_compiler(tmp_path):
    """sizeof and every offsetof / field size of every struct the binding derives from include/ovm3d.h, against what a C compiler
    makes of the same header."""
    import shutil
    import subprocess
    from ovmono3d_amd import lib
    assert len(lib.STRUCTS) >= 32
    prints = []
    for name, s in lib.STRUCTS.items():
        prints.append(f'  printf("{name} - %zu 0\\n", sizeof({name}));')
        prints += [f'  printf("{name} {f} %zu %zu\\n", sizeof((({name}*)0)->{f}), offsetof({name}, {f}));' for f, *_ in s._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include "ovm3d.h"\nint main(void) {\n' + "\n".join(prints) + "\n  return 0;\n}\n")
    cc = next((c for c in ("cc", "gcc", "clang", "/opt/rocm/lib/llvm/bin/clang") if shutil.which(c)), None)
    assert cc, "no C compiler (cc, gcc, clang, ROCm's clang) to check the layouts with"
    subprocess.run([cc, "-I", os.path.join(ROOT, "include"), "-o", str(tmp_path / "layout"), str(src)], check=True)
    compiled = [tuple(line.split()) for line in subprocess.run([str(tmp_path / "layout")], check=True, capture_output=True,
                                                               text=True).stdout.splitlines()]
    derived = []
    for name, s in lib.STRUCTS.items():
        derived.append((name, "-", str(C.sizeof(s)), "0"))
        derived += [(name, f, str(getattr(s, f).size), str(getattr(s, f).offset)) for f, *_ in s._fields_]
    assert len(compiled) > 300 and compiled == derived, [x for x in zip(compiled, derived) if x[0] != x[1]][:5]


_GOOD = "#define OVM_N 2\ntypedef struct OvmA { int32_t x[OVM_N]; const float* p; } OvmA;\nint ovm_f(const OvmA* a, int64_t n);\n"


def test_parser_takes_a_plain_header():
    """the control for the strictness cases below: the same kind of text without the offending line is bound"""
    from ovmono3d_amd import lib
    abi = lib.parse_header(_GOOD)
    assert abi.constants == {"OVM_N": 2} and list(abi.structs) == ["OvmA"] and C.sizeof(abi.structs["OvmA"]) == 16
    assert abi.functions["ovm_f"][0] is C.c_int and abi.functions["ovm_f"][1][1] is C.c_int64


@pytest.mark.parametrize("what,bad", [
    ("unknown type", "typedef struct OvmB { foo_t x; } OvmB;"),
    ("unknown type behind a pointer", "int ovm_g(const OvmNope* p);"),
    ("union member", "typedef struct OvmB { union { int32_t i; float f; } u; } OvmB;"),
    ("union", "typedef union OvmU { int32_t i; float f; } OvmU;"),
    ("bit-field", "typedef struct OvmB { uint32_t a : 3; uint32_t b : 29; } OvmB;"),
    ("function-pointer parameter", "int ovm_g(void (*done)(int32_t), int32_t n);"),
    ("function-pointer field", "typedef struct OvmB { void (*done)(int32_t); } OvmB;"),
    ("struct used before its definition", "typedef struct OvmB { OvmC c[2]; } OvmB;\ntypedef struct OvmC { int32_t x; } OvmC;"),
    ("unknown array dimension", "typedef struct OvmB { int32_t x[OVM_M]; } OvmB;"),
    ("unknown directive", "#define OVM_F 1.5f"),
    ("unknown return type", "float ovm_g(int32_t n);"),
    ("declaration without an end", "int ovm_g(int32_t n)"),
])
def test_parser_refuses_what_it_does_not_understand(what, bad):
    from ovmono3d_amd import lib
    with pytest.raises(lib.HeaderError, match=r"ovm3d\.h:4: "):           # _GOOD has three lines: the error names the fourth
        lib.parse_header(_GOOD + bad + "\n")


def test_struct_pointer_parameters_take_addresses_and_only_their_own_struct():
    """from_param alone, no library call: the one rule for `T*` parameters, on a parameter the callers hand a device address
    (OvmDet3D* out of ovm_cube_forward) and on one they hand a host struct (OvmConfig* of ovm_create)."""
    from ovmono3d_amd import lib
    out, cfg = lib.FUNCTIONS["ovm_cube_forward"][1][9], lib.FUNCTIONS["ovm_create"][1][0]
    assert out.struct is lib.OvmDet3D and cfg.struct is lib.OvmConfig
    for p, right, wrong in ((out, lib.OvmDet3D, lib.OvmEvalCell), (cfg, lib.OvmConfig, lib.OvmSamConfig)):
        for ok in (None, 0, 0x7F0000001000, C.c_void_p(4096), right(), C.byref(right()), C.pointer(right()), (right * 3)()):
            p.from_param(ok)
        for bad in (wrong(), C.byref(wrong()), C.pointer(wrong()), (wrong * 3)(), C.c_int32(1), C.byref(C.c_int32(1)), 1.0, b"x", "x"):
            with pytest.raises((TypeError, C.ArgumentError)):
                p.from_param(bad)
    # the other kinds of parameter and result
    rt, at = lib.FUNCTIONS["ovm_debug_copy"]            # int64_t (OvmHandle*, const char*, float*, int64_t, ovm_stream_t)
    assert rt is C.c_int64 and at == [C.c_void_p, C.c_char_p, C.c_void_p, C.c_int64, C.c_void_p]
    assert lib.FUNCTIONS["ovm_last_error"] == (C.c_char_p, [C.c_void_p]) and lib.FUNCTIONS["ovm_version"] == (C.c_char_p, [])
    assert lib.FUNCTIONS["ovm_host_jpeg_info"][1][:2] == [C.c_void_p, C.c_size_t]
    assert lib.FUNCTIONS["ovm_create"][1][1:] == [lib.FUNCTIONS["ovm_sam_create"][1][1], C.c_int32, C.c_int32, C.c_void_p]      # OvmHandle**
    assert lib.FUNCTIONS["ovm_eval_iou2d"][1][5] is C.c_double and lib.FUNCTIONS["ovm_op_nms"][1][3] is C.c_float


def test_version_and_error_strings():
    from ovmono3d_amd import lib
    L = lib.load()
    assert b"libovm3d" in L.ovm_version()
    assert L.ovm_last_error(None) == b"null handle"


def test_create_rejects_bad_config_without_gpu_work():
    """Argument validation happens before any device call."""
    from ovmono3d_amd import lib
    L = lib.load()
    cfg = lib.OvmConfig()
    cfg.embed_dim, cfg.depth, cfg.heads, cfg.canvas = 100, 1, 1, 225     # canvas not a multiple of 14
    cfg.precision, cfg.max_batch, cfg.max_rois, cfg.fpn_channels = 1, 1, 1, 256
    h = C.c_void_p()
    rc = L.ovm_create(C.byref(cfg), None, 0, 0, C.byref(h))
    assert rc == -1
    assert b"invalid config" in L.ovm_last_error(h)
    L.ovm_destroy(h)


def test_missing_library_fails_loudly(monkeypatch, tmp_path):
    from ovmono3d_amd import lib
    monkeypatch.setattr(lib, "_lib", None)
    monkeypatch.setattr(lib, "LIB_PATH", str(tmp_path / "nope.so"))
    try:
        lib.load()
    except RuntimeError as e:
        assert "no CPU fallback" in str(e)
    else:
        raise AssertionError("load() must raise when the shared object is absent")


def test_every_tune_key_is_documented_and_unknown_keys_are_refused():
    """ovm_tune_set is part of the C surface: every key csrc/ops.hip accepts is described in include/ovm3d.h, and a key it does not
    know is an error, not a silent no-op (a typo in OVM_TUNE must not pass for a measurement of the default)."""
    from ovmono3d_amd import lib
    ops = open(os.path.join(ROOT, "ovmono3d_amd", "csrc", "ops.hip")).read()
    hdr = open(os.path.join(ROOT, "include", "ovm3d.h")).read()
    keys = sorted(set(re.findall(r'!strcmp\(key, "([a-z0-9_]+)"\)', ops)))
    assert len(keys) >= 25
    missing = [k for k in keys if not re.search(r"\b" + k + r"\b", hdr)]
    assert not missing, f"tune keys without a line in include/ovm3d.h: {missing}"
    L = lib.load()
    assert L.ovm_tune_set(b"no_such_knob", 1) != 0
    assert L.ovm_tune_set(None, 1) != 0
