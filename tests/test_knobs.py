"""csrc/knobs.cc on the CPU: the knob table of knobs.h (every default, variable name and parse kind, and the three rules that
are not a plain read) and the form list (order, spelling, hit counters).  tests/cpp/knobs_check.cc holds the expected values
as literals, is compiled with plain g++ together with knobs.cc and run as a child process: no GPU, no library load.  The
fused gate_up column order (w4_repack.cc: host code, but behind the project's device headers) gets a small program of its
own, built host-side by the project's compiler."""
import os
import subprocess

import pytest

from tests import cpp_check

CASES = ("defaults", "each", "special", "forms")


@pytest.fixture(scope="module")
def check_program(tmp_path_factory):
    return cpp_check.build(tmp_path_factory.mktemp("knobs"), "knobs_check",
                           [os.path.join(cpp_check.CPP, "knobs_check.cc"), os.path.join(cpp_check.CSRC, "knobs.cc")])


@pytest.mark.parametrize("case", CASES)
def test_knobs(check_program, case):
    # the program starts without any FERRUM_HIP_* variable: `defaults` also looks at what the load-time initialiser read
    env = {k: v for k, v in os.environ.items() if not k.startswith("FERRUM_HIP_")}
    cpp_check.run_case(check_program, case, env=env)


def test_gate_up_col_perm(tmp_path):
    """n = 128 gives [0..31, 64..95, 32..63, 96..127]; n = 64 and n = 256 give permutations."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    exe = tmp_path / "gate_up_perm_check"
    r = subprocess.run([hipcc, "-std=c++17", "-x", "hip", "--cuda-host-only", "-O1", "-Wall", "-Werror", "-I", cpp_check.CSRC,
                        os.path.join(cpp_check.CPP, "gate_up_perm_check.cc"), os.path.join(cpp_check.CSRC, "w4_repack.cc"),
                        "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and " 0 failed" in r.stdout, r.stdout + r.stderr
