"""fh::SeqTable (csrc/seq_table.h), the runner's sequence / KV bookkeeping, on the CPU: tests/cpp/seq_table_check.cc is
compiled with plain g++ against the host-only header and run as a child process, one case per operation.  No GPU and no
library load: the block copy behind truncate / fork is injected by the program (it records (src, dst) and can fail), which
reaches the failure paths a real card cannot be made to take.  Built with AddressSanitizer + UBSan where the toolchain
links them, plain otherwise; the assertions are the same either way."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ferrum-infer-rs_amd", "csrc")
# (runtimes linked statically: the program then starts whatever else the environment preloads into its processes)
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]
CASES = ("reserve", "prefix", "fork", "truncate", "swap", "advance")


def _gxx(args, cwd):
    return subprocess.run(["g++", "-std=c++17"] + args, cwd=cwd, capture_output=True, text=True)


@pytest.fixture(scope="module")
def check_program(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("seq_table")
    (tmp / "probe.cc").write_text("int main() { return 0; }\n")
    sanitized = (_gxx(SANITIZE + ["probe.cc", "-o", "probe"], tmp).returncode == 0 and
                 subprocess.run([str(tmp / "probe")], capture_output=True).returncode == 0)      # links, and starts here
    print("seq_table_check build:", "address + undefined sanitizers" if sanitized else "plain (the sanitizers do not link here)")
    exe = tmp / "seq_table_check"
    r = _gxx(["-O1", "-g", "-Wall", "-Wextra", "-Werror"] + (SANITIZE if sanitized else []) +
             ["-I", CSRC, os.path.join(ROOT, "tests", "cpp", "seq_table_check.cc"), "-o", str(exe)], tmp)
    assert r.returncode == 0, r.stderr
    return str(exe)


def test_headers_are_host_only(tmp_path):
    """seq_table.h and block_allocator.h each compile alone with a host compiler: no HIP header, nothing missing."""
    for hdr in ("seq_table.h", "block_allocator.h"):
        (tmp_path / "only.cc").write_text('#include "%s"\n' % hdr)
        r = _gxx(["-fsyntax-only", "-I", CSRC, "only.cc"], tmp_path)
        assert r.returncode == 0, (hdr, r.stderr)
    includes = re.findall(r'#include\s*[<"]([^>"]+)[>"]', open(os.path.join(CSRC, "seq_table.h")).read())
    assert includes and not [i for i in includes if "hip" in i or i in ("common.h", "kv_layout.h", "kernels.h", "runner.h")], includes


@pytest.mark.parametrize("case", CASES)
def test_seq_table(check_program, case):
    r = subprocess.run([check_program, case], capture_output=True, text=True, timeout=60)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "%s: " % case in r.stdout and " 0 failed" in r.stdout
