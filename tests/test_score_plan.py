"""fh::score_plan and fh::score_batch_plan (csrc/score_plan.h), the launch decisions of the scoring head — argument checks,
segments and grids, the workspace and its refusal, the distinct scored rows of a packed batch, their cut into lm_head passes,
each target's (pass, row) — on the CPU: tests/cpp/score_plan_check.cc is compiled with plain g++ against the host-only header
and run as a child process, one case per group of comparisons.  No GPU and no library load."""
import os
import re

import pytest

from tests import cpp_check

CASES = ("segments", "workspace", "passes", "roundtrip", "invalid")


@pytest.fixture(scope="module")
def check_program(tmp_path_factory):
    return cpp_check.build(tmp_path_factory.mktemp("score_plan"), "score_plan_check", [os.path.join(cpp_check.CPP, "score_plan_check.cc")])


def test_header_is_host_only(tmp_path):
    """score_plan.h compiles alone with a host compiler and includes the standard library, nothing else."""
    (tmp_path / "only.cc").write_text('#include "score_plan.h"\n')
    r = cpp_check.gxx(["-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-I", cpp_check.CSRC, "only.cc"], tmp_path)
    assert r.returncode == 0, r.stderr
    src = open(os.path.join(cpp_check.CSRC, "score_plan.h")).read()
    assert re.findall(r'#include\s*"([^"]+)"', src) == []
    system = re.findall(r'#include\s*<([^>]+)>', src)
    assert system and set(system) <= {"stddef.h", "stdint.h", "stdio.h", "algorithm", "vector"}, system


@pytest.mark.parametrize("case", CASES)
def test_score_plan(check_program, case):
    cpp_check.run_case(check_program, case)
