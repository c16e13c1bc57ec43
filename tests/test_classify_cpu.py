"""CPU tests of the classify / track-stats entry points: argument errors come back as status
codes without a device, and the facade's classify program builds."""
import ctypes
import os
import re
import subprocess

from conftest import PKG, ROOT


def test_null_arguments_are_rejected_without_device():
    import picp_amd
    L = picp_amd.lib()
    counts = (ctypes.c_int64 * 3)()
    us = ctypes.c_float(0)
    n = ctypes.c_int64(0)
    assert L.picp_classify(None, 3000.0, None, None, None, None, counts) == picp_amd.ERR_ARG
    assert L.picp_batch_classify(None, 3000.0, None, None, None, None, None, counts) == picp_amd.ERR_ARG
    assert L.picp_batch_classify_time(None, 3000.0, 1, ctypes.byref(us)) == picp_amd.ERR_ARG
    assert L.picp_vo_set_track_stats(None, 1) == picp_amd.ERR_ARG
    assert L.picp_vo_get_map_stats(None, 0, 0, None, None, ctypes.byref(n)) == picp_amd.ERR_ARG
    assert L.picp_last_error()
    # a null counts is rejected before the handle is touched (any non-null pointer stands in)
    fake = ctypes.c_void_p(ctypes.addressof(counts))
    assert L.picp_classify(fake, 3000.0, None, None, None, None, None) == picp_amd.ERR_ARG
    assert L.picp_batch_classify(fake, 3000.0, None, None, None, None, None, None) == picp_amd.ERR_ARG


def test_header_declares_the_states_and_keeps_the_abi_version():
    src = open(os.path.join(ROOT, "include", "picp_c.h")).read()
    for name, val in (("PICP_CORR_SKIPPED", 0), ("PICP_CORR_INLIER", 1), ("PICP_CORR_OUTLIER", 2)):
        assert re.search(r"#define %s\s+%d\b" % (name, val), src), name
    import picp_amd
    assert (picp_amd.CORR_SKIPPED, picp_amd.CORR_INLIER, picp_amd.CORR_OUTLIER) == (0, 1, 2)
    assert picp_amd.lib().picp_abi_version() == 3  # new symbols only


def test_facade_classify_program_compiles(tmp_path):
    """include/pr/picp_solver.h's classify / inliers compile from plain host C++ (-Wall -Wextra
    -Werror), against the library."""
    out = tmp_path / "classify_main"
    cmd = [os.environ.get("CXX", "g++"), "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-Wno-ignored-qualifiers",
           "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "classify_facade", "classify_main.cpp"),
           "-L" + os.path.join(PKG, "lib"), "-lpicp_amd", "-Wl,-rpath," + os.path.join(PKG, "lib"), "-o", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    # without an argument it prints its usage and touches no device
    r = subprocess.run([str(out)], capture_output=True, text=True)
    assert r.returncode == 2 and "usage" in r.stderr
    assert os.path.exists(os.path.join(PKG, "bin", "classify_main"))  # built by the default target
