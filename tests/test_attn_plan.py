"""fh::attn_plan (csrc/attn_plan.h), the launch decision of paged attention — resident / flash / row-split / KV-split, the split
count and its workspace fallback, the compact-grid bound, 4 or 8 waves — on the CPU: tests/cpp/attn_plan_check.cc is compiled
with plain g++ against the host-only header and run as a child process, one case per group of thresholds.  No GPU and no
library load; the GPU tests reach a few points of this decision space through forms.require, this one walks each side of every
comparison.  Built with AddressSanitizer + UBSan where the toolchain links them, plain otherwise; the assertions are the same
either way."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ferrum-infer-rs_amd", "csrc")
# (runtimes linked statically: the program then starts whatever else the environment preloads into its processes)
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]
CASES = ("forms", "thresholds", "splits", "heads", "knobs", "compact")


def _gxx(args, cwd):
    return subprocess.run(["g++", "-std=c++17"] + args, cwd=cwd, capture_output=True, text=True)


@pytest.fixture(scope="module")
def check_program(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("attn_plan")
    (tmp / "probe.cc").write_text("int main() { return 0; }\n")
    sanitized = (_gxx(SANITIZE + ["probe.cc", "-o", "probe"], tmp).returncode == 0 and
                 subprocess.run([str(tmp / "probe")], capture_output=True).returncode == 0)      # links, and starts here
    print("attn_plan_check build:", "address + undefined sanitizers" if sanitized else "plain (the sanitizers do not link here)")
    exe = tmp / "attn_plan_check"
    r = _gxx(["-O1", "-g", "-Wall", "-Wextra", "-Werror"] + (SANITIZE if sanitized else []) +
             ["-I", CSRC, os.path.join(ROOT, "tests", "cpp", "attn_plan_check.cc"), "-o", str(exe)], tmp)
    assert r.returncode == 0, r.stderr
    return str(exe)


def test_header_is_host_only(tmp_path):
    """attn_plan.h compiles alone with a host compiler and includes knobs.h and the standard library, nothing else."""
    (tmp_path / "only.cc").write_text('#include "attn_plan.h"\n')
    r = _gxx(["-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-I", CSRC, "only.cc"], tmp_path)
    assert r.returncode == 0, r.stderr
    src = open(os.path.join(CSRC, "attn_plan.h")).read()
    assert re.findall(r'#include\s*"([^"]+)"', src) == ["knobs.h"]
    system = re.findall(r'#include\s*<([^>]+)>', src)
    assert system and not [i for i in system if "hip" in i], system
    knobs = re.findall(r'#include\s*[<"]([^>"]+)[>"]', open(os.path.join(CSRC, "knobs.h")).read())
    assert not [i for i in knobs if "hip" in i or i.endswith(".h") and i not in ("stdint.h", "stddef.h")], knobs


@pytest.mark.parametrize("case", CASES)
def test_attn_plan(check_program, case):
    r = subprocess.run([check_program, case], capture_output=True, text=True, timeout=60)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "%s: " % case in r.stdout and " 0 failed" in r.stdout
