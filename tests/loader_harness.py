"""The ONNX loader as a stand-alone sanitized program, for tests/test_cpu_fuzz.py and
tests/test_cpu_skip.py: go2_onnx_controller_amd/csrc/onnx_model.cpp built host-only with
-fsanitize=address,undefined -fno-sanitize-recover=all beside tests/cpp/fuzz_loader.cpp
(parse_onnx + inspect_json, exactly what go2pi_inspect_model runs) and run directly on files.
"""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

EXE = os.path.join(ROOT, "build", "fuzz_loader_asan")
SRC = os.path.join(ROOT, "go2_onnx_controller_amd", "csrc")


@pytest.fixture(scope="module")
def harness():
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    tmp = f"{EXE}.tmp{os.getpid()}"  # (each importing module builds it: never a half-written program)
    subprocess.run(["g++", "-std=c++20", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-fno-omit-frame-pointer", "-I" + SRC, os.path.join(ROOT, "tests", "cpp", "fuzz_loader.cpp"),
                    os.path.join(SRC, "onnx_model.cpp"), "-o", tmp], check=True)
    os.replace(tmp, EXE)
    return EXE


def run(exe, paths):
    """One output line per path ("ok ..." / "error ..."); any sanitizer report fails."""
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:verify_asan_link_order=0",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe] + [str(p) for p in paths], capture_output=True, text=True, errors="replace", timeout=300, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
    lines = r.stdout.splitlines()
    assert len(lines) == len(paths)
    return lines


def varint(v):
    v &= (1 << 64) - 1
    out = bytearray()
    while True:
        b = v & 0x7F
        v >>= 7
        out.append(b | (0x80 if v else 0))
        if not v:
            return bytes(out)
