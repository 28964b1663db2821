"""CPU: the bookkeeping of the unconditional code-path cache (csrc/uncond_cache.h) - budget and LRU order, key inequality on each key
field, a busy slot is never reused, an oversize entry, budget 0, invalidation by a rebind.  The checks are a stand-alone C++ program
(tests/uncond_cache_check.cpp) built with AddressSanitizer and UBSan and run as a process of its own; the header has no HIP in it."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


def _compiler():
    for c in (os.environ.get("CXX"), "g++", "clang++", "/opt/rocm/llvm/bin/clang++"):
        if c and shutil.which(c):
            return shutil.which(c)
    return None


def test_uncond_cache_bookkeeping_under_sanitizers(tmp_path):
    cxx = _compiler()
    assert cxx, "no host C++ compiler found (g++, clang++ or ROCm's clang++)"
    exe = str(tmp_path / "uncond_cache_check")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           os.path.join(HERE, "uncond_cache_check.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "uncond_cache_check ok" in r.stdout
