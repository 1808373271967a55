"""CPU check of the scope-owned resources of the host launch code (csrc/pbh_scope.h): the generic
holder behind the scratch buffers, setup-table refs and generated-column handles, instantiated
with a counting release (tests/native/scope_host.cpp) and built as a stand-alone program with
AddressSanitizer and UBSan on the host side.  Each case must release exactly once, on the stream
last set: scope exit, move construction, move assignment over a live holder, explicit reset, an
early return from a function holding two, a vector of holders destroyed in reverse, and an empty
holder (never).  No GPU call is made."""

import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "native", "scope_host.cpp")
OUT = os.path.join(HERE, "native", "_build", "scope_host")

CASES = ["scope exit", "scope exit on the stream last set", "move construction",
         "move assignment over a live holder: the old one",
         "move assignment: the moved one, once, with its stream set after", "explicit reset",
         "early return from a function holding two", "a vector of holders destroyed in reverse",
         "empty holders release nothing"]


def test_holder_releases_exactly_once():
    hipcc = "/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else shutil.which("hipcc")
    if hipcc is None:
        pytest.skip("hipcc not available")
    csrc = os.path.join(ROOT, "probabilit_amd", "csrc")
    deps = [SRC] + [os.path.join(csrc, f) for f in ("pbh_scope.h", "pbh_error.h", "pbh_common.h")]
    if not os.path.exists(OUT) or any(os.path.getmtime(d) > os.path.getmtime(OUT) for d in deps):
        os.makedirs(os.path.dirname(OUT), exist_ok=True)
        subprocess.run([hipcc, "-O1", "-g", "-std=c++17", "-Xarch_host", "-fsanitize=address,undefined",
                        "-Xarch_host", "-fno-sanitize-recover=undefined", "-I", csrc,
                        "-I", os.path.join(ROOT, "include"), SRC, "-o", OUT], check=True, capture_output=True)
    r = subprocess.run([OUT], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    for case in CASES:
        assert f"{case}: ok" in r.stdout, (case, r.stdout)
    assert "FAILED" not in r.stdout and "all ok" in r.stdout
