"""The replica estimator and the replica runs as a boundary, checked without a GPU: libfries_hip.so exports fries_h_dot, include/fries_hip.h
declares it and its result struct, the Python layer lists and wraps it, fries_amd.replicas exists, and frisys_mol_hip refuses the
--replicas combinations it cannot run before it touches a device."""
import ctypes
import os
import re
import subprocess

from fries_amd import build, engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_fries_h_dot():
    assert os.path.exists(engine.LIB_PATH), "libfries_hip.so has not been built"
    assert hasattr(ctypes.CDLL(engine.LIB_PATH), "fries_h_dot")


def test_header_declares_the_call_and_its_result():
    with open(os.path.join(ROOT, "include", "fries_hip.h")) as f:
        header = f.read()
    assert re.search(r"\bint\s+fries_h_dot\s*\(\s*fries_ctx\s*\*\s*a\s*,\s*fries_ctx\s*\*\s*b\s*,\s*fries_hdot_result\s*\*\s*out\s*\)\s*;", header)
    m = re.search(r"typedef\s+struct\s*\{([^}]*)\}\s*fries_hdot_result\s*;", header)
    assert m, "struct fries_hdot_result is not declared"
    body = " ".join(m.group(1).split())
    assert body == "double h, ovlp, abs_sum; uint64_t n_src, n_terms, n_hits;", body
    # the header comment names what the call stands in for and the threading contract
    for phrase in ("calc_h_dot", "molecule.cpp:667-885", "DistVec::internal_dot", "on another thread"):
        assert phrase in header, phrase


def test_python_layer_lists_and_wraps_it():
    assert "fries_h_dot" in engine.EXPORTS
    assert callable(getattr(engine.FriEngine, "h_dot", None))
    assert callable(getattr(engine.FriEngine, "variational_energy", None))
    assert ctypes.sizeof(engine.HdotResult) == 48
    assert engine.HDot._fields == ("h", "ovlp", "abs_sum", "n_src", "n_terms", "n_hits")
    from fries_amd.replicas import FriReplicas
    for meth in ("iterate", "pair_estimates", "close"):
        assert callable(getattr(FriReplicas, meth, None)), meth


def _driver(*extra, env=None):
    assert os.path.exists(build.DRIVER), "frisys_mol_hip has not been built"
    cmd = [build.DRIVER, "--fcidump_path", os.path.join(ROOT, "no_such_dir", "no.FCIDUMP"), "--vec_nonz", "10", "--mat_nonz", "10", "--max_dets", "100",
           "--max_iter", "1", *extra]
    return subprocess.run(cmd, capture_output=True, text=True, timeout=60, env=env)


def test_driver_refuses_replicas_with_ranks_before_touching_a_device():
    res = _driver("--replicas", "2", "--ranks", "2", "--seed", "1")
    assert res.returncode != 0
    assert "--replicas and --ranks exclude each other" in res.stderr, res.stderr


def test_driver_refuses_replicas_without_a_seed():
    res = _driver("--replicas", "2")
    assert res.returncode != 0
    assert "--replicas needs --seed" in res.stderr, res.stderr


def test_driver_refuses_the_other_replica_combinations():
    res = _driver("--replicas", "2", "--seed", "1", "--load_dir", "somewhere/")
    assert res.returncode != 0 and "--load_dir" in res.stderr, res.stderr
    res = _driver("--replicas", "2", "--seed", "1", env=dict(os.environ, WORLD_SIZE="2", RANK="0"))
    assert res.returncode != 0 and "WORLD_SIZE" in res.stderr, res.stderr
    for bad in ("0", "17"):
        res = _driver("--replicas", bad, "--seed", "1")
        assert res.returncode != 0 and "between 1 and 16" in res.stderr, res.stderr
    res = _driver("--repl_every", "5", "--seed", "1")
    assert res.returncode != 0 and "--repl_every needs --replicas" in res.stderr, res.stderr
