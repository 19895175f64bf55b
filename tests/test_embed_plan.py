"""fh::embed_plan (csrc/embed_plan.h), the launch decision of the embedding tail — argument checks, chunks per span, the
workspace the partials take and the fallback to fewer chunks, the grids — on the CPU: tests/cpp/embed_plan_check.cc is compiled
with plain g++ against the host-only header and run as a child process, one case per group of comparisons.  No GPU and no
library load."""
import os
import re

import pytest

from tests import cpp_check

CASES = ("chunks", "workspace", "independent", "invalid")


@pytest.fixture(scope="module")
def check_program(tmp_path_factory):
    return cpp_check.build(tmp_path_factory.mktemp("embed_plan"), "embed_plan_check", [os.path.join(cpp_check.CPP, "embed_plan_check.cc")])


def test_header_is_host_only(tmp_path):
    """embed_plan.h compiles alone with a host compiler and includes the standard library, nothing else."""
    (tmp_path / "only.cc").write_text('#include "embed_plan.h"\n')
    r = cpp_check.gxx(["-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-I", cpp_check.CSRC, "only.cc"], tmp_path)
    assert r.returncode == 0, r.stderr
    src = open(os.path.join(cpp_check.CSRC, "embed_plan.h")).read()
    assert re.findall(r'#include\s*"([^"]+)"', src) == []
    system = re.findall(r'#include\s*<([^>]+)>', src)
    assert system and set(system) <= {"stddef.h", "stdint.h", "stdio.h"}, system


@pytest.mark.parametrize("case", CASES)
def test_embed_plan(check_program, case):
    cpp_check.run_case(check_program, case)
