"""CPU-only checks of the drop-in boundary: libwtk_hip.so builds, loads, exports every symbol that
include/wtk_hip.h declares, and its own conv table equals the Python-side spec.  No compute calls."""
import ctypes
import os
import re

import pytest

from wtracker_amd import hip
from wtracker_amd import yolo_spec as ys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_symbols():
    text = open(os.path.join(ROOT, "include", "wtk_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(wtk_[a-z0-9_]+)\s*\(", text)))


def test_header_and_binding_list_agree():
    assert header_symbols() == sorted(hip.SYMBOLS)


def test_library_exports_every_declared_symbol(hip_lib):
    for name in header_symbols():
        assert hasattr(hip_lib, name), name
    assert hip_lib.wtk_abi_version() == 7
    assert hip_lib.wtk_last_error() is not None
    assert hip_lib.wtk_device_count() >= 0


C_KINDS = {"int": "i32", "int32_t": "i32", "int64_t": "i64", "size_t": "size", "float": "f32", "double": "f64", "void": "void"}
CTYPES_KINDS = {ctypes.c_int32: "i32", ctypes.c_int64: "i64", ctypes.c_size_t: "size", ctypes.c_float: "f32", ctypes.c_double: "f64", None: "void"}


def header_kind(decl: str, is_param: bool) -> str:
    """The kind of one C declaration ("const float *x_dev", "int64_t ld", the return type "const char *"): "ptr" or the scalar's own."""
    if "*" in decl:
        return "ptr"
    words = [w for w in decl.split() if w != "const"]
    return C_KINDS[words[0]] if len(words) == 1 + is_param else "?" + decl  # (one type word, then the parameter's name)


def ctypes_kind(t) -> str:
    if t in (ctypes.c_void_p, ctypes.c_char_p) or (isinstance(t, type) and issubclass(t, ctypes._Pointer)):
        return "ptr"
    return CTYPES_KINDS.get(t, "?" + repr(t))


def test_binding_argument_counts_match_the_header(hip_lib):
    """Every prototype of include/wtk_hip.h against the ctypes `restype` / `argtypes` wtracker_amd.hip.load() declares, kind by kind (pointer,
    int32, int64, size_t, float, double): a parameter added to one side only, or an int32 where the header has int64_t, would otherwise surface
    as a corrupted call on the GPU box."""
    text = open(os.path.join(ROOT, "include", "wtk_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    protos = re.findall(r"^([A-Za-z_][\w \t]*?[\s*])(wtk_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;", text, flags=re.S | re.M)
    assert [n for _, n, _ in protos] == hip.SYMBOLS  # (the table keeps the header's order)
    assert sorted(n for _, n, _ in protos) == header_symbols()
    for ret, name, params in protos:
        p = params.strip()
        want = [] if p in ("", "void") else [header_kind(d, True) for d in p.split(",")]
        fn = getattr(hip_lib, name)
        assert fn.argtypes is not None, name
        assert [ctypes_kind(t) for t in fn.argtypes] == want, (name, want, fn.argtypes)
        assert ctypes_kind(fn.restype) == header_kind(ret, False), (name, ret, fn.restype)
    restype, argtypes = hip.SIGNATURES["wtk_replay_scratch_doubles"]
    assert (restype, list(argtypes)) == (ctypes.c_int64, [ctypes.c_int32, ctypes.c_int64])  # (the table itself is what load() applied)


def test_every_environment_switch_is_documented():
    """Every WTK_* variable the library reads has a row in README's "Environment switches" table; the retired ones are gone from both."""
    csrc = os.path.join(ROOT, "wtracker_amd", "csrc")
    src = "".join(open(os.path.join(csrc, f)).read() for f in sorted(os.listdir(csrc)) if f.endswith((".hip", ".h")))
    read = set(re.findall(r"\b(?:getenv|env_int)\(\s*\"(WTK_[A-Z0-9_]+)\"", src))
    assert {"WTK_LATENCY_PLAN", "WTK_NO_SK_MIXED", "WTK_SMALL_NARROW", "WTK_SEGV_BACKTRACE"} <= read, read
    readme = open(os.path.join(ROOT, "README.md")).read()
    table = readme.split("## Environment switches", 1)[1].split("\n## ", 1)[0]
    documented = set(re.findall(r"`(WTK_[A-Z0-9_]+)", table))
    assert read <= documented, sorted(read - documented)
    retired = ("GRAPH", "GRAPH_HOST", "GRAPH_VIEWS", "GRAPH_MAX_BATCH", "SK_MIXED_MAX_PX", "SK_PLAN_ATOMS", "SK_SINGLE_MAX", "SK_SLICE_STEPS",
               "SK_INKERNEL_MAX_KB", "SK_VERBOSE")
    for name in ("WTK_" + r for r in retired):
        assert not re.search(r"\b%s\b" % name, src), name
        assert not re.search(r"\b%s\b" % name, readme), name


@pytest.mark.parametrize("scale,nc", [("n", 1), ("s", 1), ("s", 80), ("m", 3), ("l", 1), ("x", 1)])
def test_conv_table_matches_python_spec(hip_lib, scale, nc):
    w, d, m = ys.scale_params(scale)
    assert hip.yolo_conv_table(w, d, m, nc) == ys.conv_table(scale, nc)


def test_bad_scale_is_reported(hip_lib):
    assert hip_lib.wtk_yolo_conv_count(ctypes.c_float(0.0), ctypes.c_float(0.33), 1024, 1) == -1
    with pytest.raises(hip.WtkError):
        hip.yolo_conv_table(0.5, 0.33, 1024, 0)


def test_product_path_fails_loudly_without_gpu(hip_lib):
    """No CPU fallback: with no visible device every create call must raise, never compute."""
    if hip.device_count() > 0:
        pytest.skip("a GPU is visible")
    import numpy as np

    with pytest.raises(hip.WtkError, match="GPU"):
        hip.HipMLP([(np.zeros((2, 28), np.float32), np.zeros(2, np.float32), False)] * 2, 0, 0)
    with pytest.raises(hip.WtkError, match="GPU"):
        hip.HipYolo(ys.synthetic_weights("n", 1), (64, 64), 1, width=0.25)


def test_communicator_fails_loudly_without_gpu(hip_lib):
    if hip.device_count() > 0:
        pytest.skip("a GPU is visible")
    with pytest.raises(hip.WtkError, match="GPU"):
        hip.WtkComm(0, 0, 1, bytes(hip.COMM_ID_BYTES))
    with pytest.raises(hip.WtkError, match="128"):
        hip.WtkComm(0, 0, 1, b"short")


def test_no_product_module_imports_the_oracle():
    pkg = os.path.join(ROOT, "wtracker_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".h")):
                src = open(os.path.join(dirpath, f)).read()
                assert not re.search(r"^\s*(from|import)\s+oracle\b", src, flags=re.M), f


def test_one_hip_runtime_whatever_the_import_order(hip_lib):
    """libwtk_hip.so loaded BEFORE torch must not bring a second HIP / HSA runtime into the process (the one that initialises second
    would see no GPU): hip.load() maps torch's copies first, so both orders end with exactly one libamdhip64 and one libhsa-runtime64."""
    import subprocess
    import sys

    probe = ("import sys; sys.path.insert(0, %r); %s; "
             "print(sorted(set(l.split()[-1] for l in open('/proc/self/maps') if 'amdhip64' in l or 'hsa-runtime64' in l)))")
    for order in ("from wtracker_amd import hip; hip.load(); import torch", "import torch; from wtracker_amd import hip; hip.load()"):
        out = subprocess.run([sys.executable, "-c", probe % (ROOT, order)], capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stderr[-2000:]
        libs = eval(out.stdout.strip().splitlines()[-1])
        assert len([p for p in libs if "amdhip64" in p]) == 1 and len([p for p in libs if "hsa-runtime64" in p]) == 1, (order, libs)


def test_load_leaves_the_environment_alone(hip_lib):
    """hip.load() used to write GPU_MAX_HW_QUEUES=8 into os.environ, which every child process inherits (rank processes sharing one
    device then asked for eight hardware queues each).  The request is now the explicit hip.request_hw_queues(): after load() neither this process
    nor a child spawned from it sees the variable unless somebody asked for it."""
    import subprocess
    import sys

    code = ("import os, sys; sys.path.insert(0, %r); os.environ.pop('GPU_MAX_HW_QUEUES', None); from wtracker_amd import hip; hip.load(); "
            "assert 'GPU_MAX_HW_QUEUES' not in os.environ; "
            "import subprocess; print(subprocess.run([sys.executable, '-c', \"import os; print(os.environ.get('GPU_MAX_HW_QUEUES'))\"], capture_output=True, text=True).stdout.strip()); "
            "assert hip.request_hw_queues(8) and os.environ['GPU_MAX_HW_QUEUES'] == '8' and not hip.request_hw_queues(5) and os.environ['GPU_MAX_HW_QUEUES'] == '8'") % ROOT
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    assert out.stdout.strip().splitlines()[-1] == "None"
