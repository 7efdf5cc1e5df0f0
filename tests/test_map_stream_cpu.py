"""The queue behind cs_map_submit / cs_map_collect (compseed_amd/csrc/map_stream.hpp): the slot ring, its three workers, the cap, the
order, the error hand-over and the life of a collected result decide which batch runs where and when, never what a batch returns, so no
parity test sees them.  tests/cpp/map_stream_check.cpp drives the header alone with stub parts on real threads through a few thousand
random schedules; it is plain C++ and needs no GPU."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))


def test_map_stream_check_program(tmp_path):
    exe = str(tmp_path / "map_stream_check")
    src = os.path.join(HERE, "cpp", "map_stream_check.cpp")
    c = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-pthread", "-o", exe, src], capture_output=True, text=True)
    assert c.returncode == 0 and not c.stderr, c.stderr                      # (no warnings either)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "DIFFERS" not in r.stdout and r.stdout.rstrip().endswith("0 case(s) differ")
    assert r.stdout.count("  ok\n") == 8                                    # every family of schedules was run
    assert sum(int(l.split()[-3]) for l in r.stdout.splitlines() if l.endswith("schedules  ok")) >= 3000
