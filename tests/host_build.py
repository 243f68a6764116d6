"""The host builds of the tests: a stand-alone program tests/host/NAME.cpp (its own `main`) around a csrc/*_core.h, compiled with the host
compiler and run as a child process."""
import os
import shutil
import struct
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SANITIZE = ['-fsanitize=address,undefined', '-fno-sanitize-recover=undefined']


def compile_host_check(tmp_path, name, flags=(), start_args=(), suffix=''):
    """tests/host/`name`.cpp -> (exe, sanitized): with -fsanitize=address,undefined where that links AND the program starts (exit status 0
    on a case file of zero cases, `exe EMPTY *start_args`), the runtimes inside the program where the compiler can; plain otherwise."""
    cxx = os.environ.get('CXX') or shutil.which('g++') or shutil.which('clang++') or shutil.which('c++')
    if cxx is None:
        pytest.fail('no host C++ compiler (g++, clang++ or c++) to compile tests/host/%s.cpp' % name)
    exe = str(tmp_path / (name + suffix))
    base = [cxx, '-std=c++17', '-O1', '-g', '-Wall', '-Werror', '-o', exe, os.path.join(ROOT, 'tests', 'host', name + '.cpp')] + list(flags)
    empty = str(tmp_path / 'empty.bin')
    with open(empty, 'wb') as f:
        f.write(struct.pack('<q', 0))
    for extra in (SANITIZE + ['-static-libasan', '-static-libubsan'], SANITIZE + ['-static-libsan'], SANITIZE):
        r = subprocess.run(base + extra, capture_output=True, text=True)
        if r.returncode == 0 and subprocess.run([exe, empty] + list(start_args), capture_output=True).returncode == 0:
            return exe, True
    r = subprocess.run(base, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe, False
