"""The part boundaries and the offset check of a host submit (compseed_amd/csrc/host_parts.hpp): they decide how fast a blocking call is,
never what it returns, so no parity test sees them.  tests/cpp/host_parts_check.cpp holds the cases; it is plain C++ and needs no GPU."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))


def test_host_parts_check_program(tmp_path):
    exe = str(tmp_path / "host_parts_check")
    src = os.path.join(HERE, "cpp", "host_parts_check.cpp")
    c = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-pthread", "-o", exe, src], capture_output=True, text=True)
    assert c.returncode == 0 and not c.stderr, c.stderr                      # (no warnings either)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "DIFFERS" not in r.stdout and r.stdout.rstrip().endswith("0 case(s) differ")
    assert r.stdout.count("  ok\n") >= 9 + 7                                # every cut row and every offsets case was run
