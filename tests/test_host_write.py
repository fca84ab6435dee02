"""mirge_amd/csrc/host_write.hpp -- the file, thread rule, ordered scheduler and read unpacking every native report
writer shares -- checked by a stand-alone program (tests/helpers/host_write_check.cpp) that includes nothing but the
header: built with plain g++ into tests/_build/ and run as a child process.  No GPU, no library."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "mirge_amd", "csrc")


def test_host_write_header(tmp_path):
    src = os.path.join(HERE, "helpers", "host_write_check.cpp")
    hdr = os.path.join(CSRC, "host_write.hpp")
    exe = os.path.join(HERE, "_build", "host_write_check")
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(src), os.path.getmtime(hdr)):
        os.makedirs(os.path.dirname(exe), exist_ok=True)
        subprocess.run(["g++", "-O1", "-std=c++17", "-pthread", "-Wall", "-I", CSRC, "-o", exe, src], check=True)
    run = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr
    assert run.stdout.strip() == "host_write ok"
