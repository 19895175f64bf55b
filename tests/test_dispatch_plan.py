"""fh::plan_batched_dispatch (csrc/moe_dispatch_plan.h), the host half of gemm_phase_batched — dispatch list → block-major
routing arrays: grouping by output displacement, the 16- versus 64-row choice, the sentinel rows, the range check — on the
CPU: tests/cpp/dispatch_plan_check.cc is compiled with plain g++ against the host-only header and run as a child process.
No GPU and no library load; the GPU test of gemm_phase_batched reaches one point of this, this one every rule."""
import os
import re

import pytest

from tests import cpp_check

CASES = ("groups", "tiles", "threshold", "empty", "refused", "order")


@pytest.fixture(scope="module")
def check_program(tmp_path_factory):
    return cpp_check.build(tmp_path_factory.mktemp("dispatch_plan"), "dispatch_plan_check",
                           [os.path.join(cpp_check.CPP, "dispatch_plan_check.cc")])


def test_header_is_host_only(tmp_path):
    """moe_dispatch_plan.h compiles alone with a host compiler and includes error.h and the standard library, nothing else."""
    (tmp_path / "only.cc").write_text('#include "moe_dispatch_plan.h"\n')
    r = cpp_check.gxx(["-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-I", cpp_check.CSRC, "only.cc"], tmp_path)
    assert r.returncode == 0, r.stderr
    src = open(os.path.join(cpp_check.CSRC, "moe_dispatch_plan.h")).read()
    assert re.findall(r'#include\s*"([^"]+)"', src) == ["error.h"]
    system = re.findall(r'#include\s*<([^>]+)>', src)
    assert system and not [i for i in system if "hip" in i], system
    assert not re.findall(r'#include', open(os.path.join(cpp_check.CSRC, "error.h")).read())


@pytest.mark.parametrize("case", CASES)
def test_dispatch_plan(check_program, case):
    cpp_check.run_case(check_program, case)
