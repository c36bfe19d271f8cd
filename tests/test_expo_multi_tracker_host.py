"""lambda-lanczos_amd/csrc/ritz_tracker.hpp — ExpoMultiTracker, the stop rule of the multi-time two-pass Exponentiator — against one
ExpoTracker per time on the same tridiagonal prefixes (tests/cpp/expo_multi_tracker_test.cpp states the properties): iteration
counts and frozen coefficients equal as bytes, `stop` exactly at the last time's stop, breakdown, a max_iteration cut, and the helper
thread.  The header builds with a plain host compiler (the HIP headers are needed for types in declarations only), once more with
the address and undefined-behaviour sanitizers, and both programs run as ordinary child processes."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lambda-lanczos_amd", "csrc")


@pytest.mark.parametrize("sanitize", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "sanitized"])
def test_expo_multi_tracker_against_single_trackers(tmp_path, sanitize):
    exe = str(tmp_path / "expo_multi_tracker_test")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wextra", "-Wno-unused-parameter",
                    "-Wno-missing-field-initializers", "-Wno-deprecated-declarations", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
                    "-I", CSRC] + sanitize +
                   [os.path.join(ROOT, "tests", "cpp", "expo_multi_tracker_test.cpp"), os.path.join(CSRC, "tridiag_host.cpp"), "-o", exe,
                    "-ldl", "-lpthread"], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stderr == "", (r.stdout[-2000:], r.stderr[-2000:])
    assert " 0 failures" in r.stdout
