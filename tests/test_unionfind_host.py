"""The union-find of mdir_amd/csrc/mdx_unionfind.h on the host: tests/unionfind_host.cpp, a stand-alone program that includes the
header under a host memory policy, runs path, star, permuted, random and clique edge sets from 8 threads and compares the roots
with a sequential union-find.  Built here with the host compiler under AddressSanitizer + UBSan and, where that links, under
ThreadSanitizer, and run as a child process: nothing is loaded into this interpreter."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

SOURCE = os.path.join(ROOT, "tests", "unionfind_host.cpp")
SETS = ("path", "star", "permuted", "random", "clique", "give-up")


def _compiler():
    for name in (os.environ.get("CXX"), "c++", "g++", "clang++"):
        path = shutil.which(name) if name else None
        if path:
            return path
    pytest.fail("no host C++ compiler (c++, g++ or clang++) on PATH")


def _build(tmp_path, name, sanitize):
    out = str(tmp_path / name)
    cmd = [_compiler(), "-std=c++17", "-O1", "-g", "-pthread", "-fsanitize=" + sanitize, "-fno-sanitize-recover=all", "-o", out, SOURCE]
    return out, subprocess.run(cmd, capture_output=True, text=True, timeout=300)


def _run(binary):
    done = subprocess.run([binary], capture_output=True, text=True, timeout=300)
    assert done.returncode == 0, done.stdout + done.stderr
    lines = done.stdout.splitlines()
    assert lines and all(line.endswith(" ok") for line in lines), done.stdout
    assert {line.split()[0] for line in lines} == set(SETS), done.stdout
    assert "Sanitizer" not in done.stderr, done.stderr


def test_unionfind_under_address_and_ub_sanitizers(tmp_path):
    binary, built = _build(tmp_path, "unionfind_asan", "address,undefined")
    assert built.returncode == 0, built.stderr
    _run(binary)


def test_unionfind_under_thread_sanitizer(tmp_path):
    """The relaxed atomics of the host policy are atomics: ThreadSanitizer must see no race in parent.  Where the toolchain
    cannot link its runtime, the address / UB build above is the whole check."""
    binary, built = _build(tmp_path, "unionfind_tsan", "thread")
    if built.returncode != 0:
        assert "tsan" in built.stderr.lower() or "thread" in built.stderr.lower(), built.stderr
        return
    probe = subprocess.run([binary], capture_output=True, text=True, timeout=300)
    if probe.returncode != 0 and not probe.stdout and "unexpected memory mapping" in probe.stderr:
        return                          # the runtime could not map its shadow memory (address-space layout): it never reached main
    _run(binary)
