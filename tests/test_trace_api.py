"""rtx_trace_device's interface (no GPU): the header declares it, librtx.so exports it, and the ctypes
prototype (raytracing_rb_amd/_abi.py, loaded by runtime.py) and the Fiddle extern (ext/rtx/lib/rtx.rb)
agree with the header's argument list."""

import ctypes as C
import os
import re

from conftest import ROOT

C_TO_CTYPES = {"rtx_context*": C.c_void_p, "int32_t": C.c_int32, "uint64_t": C.c_uint64, "const double*": C.c_void_p,
               "const int32_t*": C.c_void_p, "double*": C.c_void_p, "int32_t*": C.c_void_p, "void*": C.c_void_p}
C_TO_FIDDLE = {"rtx_context*": "void*", "int32_t": "int", "uint64_t": "unsigned long long", "const double*": "void*",
               "const int32_t*": "void*", "double*": "void*", "int32_t*": "void*", "void*": "void*"}


def _header_args():
    hdr = open(os.path.join(ROOT, "include", "rtx.h")).read()
    m = re.search(r"rtx_status\s+rtx_trace_device\(([^)]*)\);", hdr)
    assert m, "include/rtx.h does not declare rtx_trace_device"
    args = [re.sub(r"\s+", " ", a.strip()) for a in m.group(1).split(",")]
    return [re.sub(r"\s*\w+$", "", a) for a in args]              # drop the parameter names


def test_header_declares_the_call():
    assert _header_args() == ["rtx_context*", "int32_t", "uint64_t", "const double*", "const int32_t*", "double*",
                              "int32_t*", "void*"]


def test_library_exports_it_and_refuses_a_null_context():
    from raytracing_rb_amd import _abi
    lib = _abi.load_library()
    assert hasattr(lib, "rtx_trace_device")
    assert lib.rtx_trace_device(None, 1, 1, None, None, None, None, None) == 6


def test_ctypes_prototype_and_fiddle_extern_match_the_header():
    from raytracing_rb_amd import _abi, api, runtime
    args = _header_args()
    sig = {n: (r, a) for n, r, a in _abi.SIGNATURES}
    assert sig["rtx_trace_device"] == (C.c_int32, [C_TO_CTYPES[a] for a in args])
    rb = open(os.path.join(ROOT, "ext", "rtx", "lib", "rtx.rb")).read()
    assert "extern 'int rtx_trace_device(%s)'" % ", ".join(C_TO_FIDDLE[a] for a in args) in rb
    assert callable(runtime.Renderer.trace_device) and callable(api.RayTracer.trace_many)


def test_option_is_documented():
    hdr = open(os.path.join(ROOT, "include", "rtx.h")).read()
    src = open(os.path.join(ROOT, "raytracing_rb_amd", "csrc", "rtx_capi.cpp")).read()
    assert '"trace_engine"' in hdr and '"trace_engine_last"' in hdr
    m = re.search(r"#define RTX_TRACE_LEVELS_MIN_RAYS (\w+)", src)
    assert m and "RTX_TRACE_LEVELS_MIN_RAYS = %s" % m.group(1) in hdr   # the header quotes the threshold
