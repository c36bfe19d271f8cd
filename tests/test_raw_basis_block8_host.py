"""lambda-lanczos_amd/csrc/raw_basis.hpp on the records that blocks of eight Lanczos iterations leave: a stop, a flush or a
hand-over at every row of an eight-row block, with the record allocated to exactly the rows the loop fetches for that stop
(tests/cpp/raw_basis_block8_test.cpp states the cases).  Built with a plain host compiler and once more with the address and
undefined-behaviour sanitizers; both programs run as ordinary child processes."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("sanitize", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "sanitized"])
def test_raw_basis_algebra_on_eight_row_blocks(tmp_path, sanitize):
    exe = str(tmp_path / "raw_basis_block8_test")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(ROOT, "lambda-lanczos_amd", "csrc")] + sanitize +
                   [os.path.join(ROOT, "tests", "cpp", "raw_basis_block8_test.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stderr == "", (r.stdout[-2000:], r.stderr[-2000:])
    assert " 0 failures" in r.stdout
