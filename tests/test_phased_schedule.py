"""The schedule of the phased k loop (seekr_amd/csrc/gemm_phased_schedule.hpp, SEEKR_GEMM_LOOP=1) on the CPU: the function the
kernel's loop is generated from runs with recording operations for both wave groups and kt = 1 ... 9, 32, 33, 128
(tests/phased_schedule_model.cpp); equal barrier counts on every path, every read behind the counted wait that retires
exactly its buffer and a barrier both groups passed, every restage behind both groups' last reads, every N the pieces
outstanding.  A stand-alone host program under -fsanitize=address,undefined; no GPU."""
import os
import shutil
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))


def _host_compiler():
    for name in (os.environ.get("CXX"), "c++", "g++", "clang++", "/opt/rocm/llvm/bin/clang++"):
        if name and shutil.which(name):
            return shutil.which(name)
    raise AssertionError("no host C++ compiler found (CXX, c++, g++, clang++)")


def test_phased_loop_schedule_keeps_the_staging_rules(tmp_path):
    exe = str(tmp_path / "phased_schedule_model")
    src = os.path.join(HERE, "phased_schedule_model.cpp")
    build = subprocess.run([_host_compiler(), "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=undefined", src, "-o", exe], capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, build.stdout[-2000:] + build.stderr[-4000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and "phased schedule ok" in run.stdout, run.stdout[-2000:] + run.stderr[-4000:]
