"""Building the stand-alone host programs under tests/cpp/ (test_dispatch_plan.py, test_knobs.py): plain g++ against csrc/,
with AddressSanitizer + UBSan where the toolchain links them and the result starts here, plain otherwise.  The programs are
run as child processes; nothing is loaded into Python."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ferrum-infer-rs_amd", "csrc")
CPP = os.path.join(ROOT, "tests", "cpp")
# (runtimes linked statically: the program then starts whatever else the environment preloads into its processes)
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]


def gxx(args, cwd):
    return subprocess.run(["g++", "-std=c++17"] + args, cwd=cwd, capture_output=True, text=True)


def build(tmp, name, sources):
    """g++ the sources (paths, or names under tests/cpp/ and csrc/) into tmp/name; returns the program's path."""
    (tmp / "probe.cc").write_text("int main() { return 0; }\n")
    sanitized = (gxx(SANITIZE + ["probe.cc", "-o", "probe"], tmp).returncode == 0 and
                 subprocess.run([str(tmp / "probe")], capture_output=True).returncode == 0)      # links, and starts here
    print("%s build:" % name, "address + undefined sanitizers" if sanitized else "plain (the sanitizers do not link here)")
    exe = tmp / name
    r = gxx(["-O1", "-g", "-Wall", "-Wextra", "-Werror"] + (SANITIZE if sanitized else []) + ["-I", CSRC] + sources + ["-o", str(exe)], tmp)
    assert r.returncode == 0, r.stderr
    return str(exe)


def run_case(exe, case, env=None):
    r = subprocess.run([exe, case], capture_output=True, text=True, timeout=60, env=env)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "%s: " % case in r.stdout and " 0 failed" in r.stdout
