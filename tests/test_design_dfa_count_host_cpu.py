"""The host side of ``rnampnn_design_dfa_count`` on the CPU: tests/native/design_dfa_count_host_test.cpp is a stand-alone program that
includes rna-mpnn_amd/csrc/design_dfa_count.hip, supplies the library's ``fail`` and calls the entry with every argument it refuses before a
launch (and with every output null, which launches nothing), and checks the workspace and LDS formulas.  It is built with the compiler of
the library's build, with the address and undefined-behaviour sanitizers on the host side, and run as a child process (nothing is loaded
into this interpreter)."""
import os
import subprocess

from conftest import REPO


def test_design_dfa_count_host_checks(tmp_path):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    exe = str(tmp_path / "design_dfa_count_host_test")
    cmd = [hipcc, "-x", "hip", "--offload-arch=gfx950", "-std=c++17", "-O1", "-g", "-Wno-unused-value", "-Xarch_host", "-fsanitize=address,undefined",
           "-Xarch_host", "-fno-sanitize-recover=undefined", "-I", os.path.join(REPO, "rna-mpnn_amd", "csrc"),
           os.path.join(REPO, "tests", "native", "design_dfa_count_host_test.cpp"), "-o", exe]
    built = subprocess.run(cmd, capture_output=True, text=True, cwd=REPO)
    assert built.returncode == 0, built.stderr
    ran = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert ran.returncode == 0, ran.stdout + ran.stderr
    assert "design_dfa_count_host_test: ok" in ran.stdout
