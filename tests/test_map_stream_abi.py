"""cs_map_submit / cs_map_collect / cs_mapper_in_flight without a GPU: the entry points exist, refuse NULL arguments, and the cap is 3 in the
header and in the binding."""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    import compseed_amd as ca
    if not os.path.exists(ca.lib_path()):
        ca.build_library()
    return ca.load_library()


def test_the_three_entry_points_exist(lib):
    for name in ("cs_map_submit", "cs_map_collect", "cs_mapper_in_flight"):
        assert getattr(lib, name) is not None
    import compseed_amd as ca
    assert all(callable(getattr(ca.Mapper, f)) for f in ("submit", "collect", "in_flight"))


def test_null_arguments(lib):
    import compseed_amd as ca
    out = ca.binding.CSamResult(); s, f = C.c_int(7), C.c_int(7)
    assert lib.cs_map_submit(None, 0, None, None, None, None, None, None, None, 0) == -1 and b"cs_map_submit" in lib.cs_last_error()
    assert lib.cs_map_collect(None, C.byref(out)) == -1 and b"cs_map_collect" in lib.cs_last_error()
    assert lib.cs_map_collect(None, None) == -1
    assert lib.cs_mapper_in_flight(None, C.byref(s), C.byref(f)) == -1 and (s.value, f.value) == (7, 7)
    # a NULL `out` (or count) on a mapper is refused before the mapper is looked at: any non-NULL address stands in for one without a GPU
    fake = C.create_string_buffer(64)
    assert lib.cs_map_collect(C.addressof(fake), None) == -1
    assert lib.cs_mapper_in_flight(C.addressof(fake), None, C.byref(f)) == -1 and lib.cs_mapper_in_flight(C.addressof(fake), C.byref(s), None) == -1


def test_the_cap_is_three_in_header_and_binding(tmp_path):
    import compseed_amd as ca
    (tmp_path / "cap.c").write_text('#include <stdio.h>\n#include "compseed_amd.h"\nint main(void) { printf("%d\\n", (int)CS_MAP_MAX_IN_FLIGHT); return 0; }\n')
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", str(tmp_path / "cap"), str(tmp_path / "cap.c")], check=True)
    got = int(subprocess.run([str(tmp_path / "cap")], capture_output=True, text=True, check=True).stdout)
    assert got == ca.MAP_MAX_IN_FLIGHT == 3
