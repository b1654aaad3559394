"""The stepwise FRI iteration as a boundary, checked without a GPU: libfries_hip.so exports the entry points, the Python layer lists
them, include/fries_hip.h declares them, and the test consumer of include/FRIES/device_loop.hpp was built."""
import ctypes
import os
import re

from fries_amd import build, engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["fries_spawn_from_comp", "fries_dense_apply", "fries_dense_norm", "fries_dense_h_count", "fries_comp_download"]


def test_library_exports_the_stepwise_entry_points():
    assert os.path.exists(engine.LIB_PATH), "libfries_hip.so has not been built"
    lib = ctypes.CDLL(engine.LIB_PATH)
    for name in NEW:
        assert hasattr(lib, name), name


def test_entry_points_are_listed_and_declared():
    with open(os.path.join(ROOT, "include", "fries_hip.h")) as f:
        header = f.read()
    for name in NEW:
        assert name in engine.EXPORTS, name
        assert re.search(r"\bint\s+%s\s*\(\s*fries_ctx\s*\*" % name, header), name
    for meth in ("spawn_from_comp", "dense_apply", "dense_norm", "dense_h_count", "comp_download", "death_clone", "dots", "find_preserve",
                 "sys_comp", "iterate_stepwise"):
        assert callable(getattr(engine.FriEngine, meth, None)), meth


def test_device_loop_consumer_was_built():
    assert os.path.exists(os.path.join(ROOT, "include", "FRIES", "device_loop.hpp"))
    assert os.path.exists(build.DEVICE_LOOP_DRIVER), "frisys_mol_device_loop (tests/cpp/frisys_mol_device_loop.cpp) has not been built"
    assert os.access(build.DEVICE_LOOP_DRIVER, os.X_OK)
