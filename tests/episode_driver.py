"""How the CPU tests build and run a stand-alone host driver under AddressSanitizer and UndefinedBehaviorSanitizer: the compilers and flags, the
`driver` fixture of tests/episode_book_driver.cpp (the one program behind test_episode_book_build.py, test_episode_fork_build.py and
test_episode_snapshot_build.py) and the line protocol around it."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
# the sanitizer runtimes linked statically where the compiler has the choice: the program runs whatever else the process environment loads
COMPILERS = (["g++", "-static-libasan", "-static-libubsan"], [os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", "clang++")], ["g++"])


def build_driver(tmp_path_factory, name):
    """tests/<name>.cpp as a sanitized program in a temporary directory -> its path"""
    exe = str(tmp_path_factory.mktemp(name) / name)
    errors = []
    for cc in COMPILERS:
        if not shutil.which(cc[0]):
            continue
        r = subprocess.run(cc + FLAGS + ["-I", os.path.join(ROOT, "vima_amd", "csrc"), os.path.join(ROOT, "tests", name + ".cpp"), "-o", exe],
                           capture_output=True, text=True)
        if r.returncode == 0:
            return exe
        errors.append(" ".join(cc) + ":\n" + r.stderr[-2000:])
    raise AssertionError("no host compiler built the driver with -fsanitize=address,undefined:\n" + "\n".join(errors))


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return build_driver(tmp_path_factory, "episode_book_driver")


def _run(exe, ops, brief=False):
    """brief: the short plan / step, install and state lines of the fork and snapshot tests"""
    r = subprocess.run([exe] + (["brief"] if brief else []), input="".join(o + "\n" for o in ops), capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, (r.returncode, r.stderr[-3000:])      # a sanitizer report ends the program with a non-zero status
    lines = r.stdout.splitlines()
    assert len(lines) == len(ops)
    return lines


def _flags(flags):
    return " ".join("1" if f else "0" for f in flags)


def _ints(xs):
    return " ".join(str(int(x)) for x in xs)
