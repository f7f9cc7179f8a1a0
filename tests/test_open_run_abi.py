"""What tests/test_abi_exports.py does not cover of the open-run and batched-chunk entry points: the argument struct's layout as
the Python binding declares it, and the refusals that need no GPU."""
import ctypes
import os
import re

from rho_tts_amd import _native
from rho_tts_amd._native_model import RtGenerateOpenArgs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_fields(struct):
    src = open(os.path.join(ROOT, "include", "rho_tts_amd.h")).read()
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), src, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for decl in body.split(";"):
        names += [re.sub(r"[\s*]", "", n.split()[-1]) for n in decl.split(",") if n.strip()]
    return names


def test_open_args_match_the_header_field_for_field():
    assert header_fields("rt_generate_open_args") == [n for n, _ in RtGenerateOpenArgs._fields_]
    # 5 x i32 + pad, pointer, u64, 2 x rt_sampling (20 bytes), 6 x i32, pointer, i32 + pad, 8 pointers
    assert ctypes.sizeof(RtGenerateOpenArgs) == 184
    assert RtGenerateOpenArgs.h_voices.offset == 24 and RtGenerateOpenArgs.seed.offset == 32 and RtGenerateOpenArgs.h_cancel_flag.offset == 104
    assert RtGenerateOpenArgs.n_items.offset == 112 and RtGenerateOpenArgs.d_trace_predictor.offset == 176


def test_abi_version_is_unchanged_and_the_new_symbols_are_there():
    lib = _native.load_library()
    assert lib.rt_abi_version() == 6
    for name in ("rt_generate_open", "rt_generate_submit", "rt_generate_cancel_item", "rt_generate_cadence", "rt_stream_chunks"):
        assert hasattr(lib, name), name


def test_null_handles_are_refused_without_a_gpu():
    lib = _native.load_library()
    item = ctypes.c_int32(-1)
    assert lib.rt_generate_open(None, None) == _native.RT_ERR_INVALID
    assert lib.rt_generate_submit(None, None, 0, 1, 0, 0, ctypes.byref(item)) == _native.RT_ERR_INVALID and item.value == -1
    assert lib.rt_generate_cancel_item(None, 0) == _native.RT_ERR_INVALID
    assert lib.rt_generate_cadence(None) >= 1                  # (no run: the cadence the next open run takes)
    assert issubclass(_native.LengthError, RuntimeError)
    assert lib.rt_stream_chunks(None, None, 0, None, None, None, None, None, None) == _native.RT_ERR_INVALID
