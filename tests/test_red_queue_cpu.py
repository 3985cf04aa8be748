"""The ordered-reduction queue of the trainer's backward (rna-mpnn_amd/csrc/red_queue.h) on the CPU: tests/native/red_queue_test.cpp is a
stand-alone program that includes the host-only header, records the batches the queue would launch and checks spans_meet against a brute-force
intersection.  It is built with the compiler of the library's build, with the address and undefined-behaviour sanitizers on the host side, and
run as a child process (nothing is loaded into this interpreter)."""
import os
import subprocess

from conftest import REPO


def test_red_queue_host_logic(tmp_path):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    rocm_include = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(hipcc))), "include")      # hipStream_t: hip_runtime_api.h
    exe = str(tmp_path / "red_queue_test")
    cmd = [hipcc, "-x", "c++", "-std=c++17", "-O1", "-g", "-D__HIP_PLATFORM_AMD__", "-Xarch_host", "-fsanitize=address,undefined",
           "-Xarch_host", "-fno-sanitize-recover=undefined", "-isystem", rocm_include, "-I", os.path.join(REPO, "rna-mpnn_amd", "csrc"),
           os.path.join(REPO, "tests", "native", "red_queue_test.cpp"), "-o", exe]
    built = subprocess.run(cmd, capture_output=True, text=True, cwd=REPO)
    assert built.returncode == 0, built.stderr
    ran = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert ran.returncode == 0, ran.stdout + ran.stderr
    assert "red_queue_test: ok" in ran.stdout and "spans_meet:" in ran.stdout
