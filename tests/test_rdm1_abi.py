"""The one-body density matrix between replicas as a boundary, checked without a GPU: libfries_hip.so exports fries_rdm1, include/fries_hip.h
declares it and its result struct, the Python layer lists and wraps it, FriReplicas has pair_rdm1, and frisys_mol_hip refuses --repl_rdm1
without --replicas before it touches a device."""
import ctypes
import os
import re
import subprocess

from fries_amd import build, engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_fries_rdm1():
    assert os.path.exists(engine.LIB_PATH), "libfries_hip.so has not been built"
    assert hasattr(ctypes.CDLL(engine.LIB_PATH), "fries_rdm1")


def test_header_declares_the_call_and_its_result():
    with open(os.path.join(ROOT, "include", "fries_hip.h")) as f:
        header = f.read()
    assert re.search(r"\bint\s+fries_rdm1\s*\(\s*fries_ctx\s*\*\s*a\s*,\s*fries_ctx\s*\*\s*b\s*,\s*double\s*\*\s*gamma\s*(/\*.*?\*/)?\s*,\s*fries_rdm1_result\s*\*\s*out\s*\)\s*;", header)
    m = re.search(r"typedef\s+struct\s*\{([^}]*)\}\s*fries_rdm1_result\s*;", header)
    assert m, "struct fries_rdm1_result is not declared"
    body = " ".join(m.group(1).split())
    assert body == "double ovlp, abs_sum; uint64_t n_src, n_terms, n_hits;", body
    # the header comment names what the call stands in for, the diagonal it defines, the threading contract and what is out of scope
    for phrase in ("one_elec_op", "molecule.cpp:222-252", "DistVec::internal_dot", "number operator", "on another thread", "Out of scope",
                   "two-body", "weight_vec", "include/FRIES"):
        assert phrase in header, phrase


def test_python_layer_lists_and_wraps_it():
    assert "fries_rdm1" in engine.EXPORTS
    assert callable(getattr(engine.FriEngine, "rdm1", None))
    assert ctypes.sizeof(engine.Rdm1Result) == 40
    assert [f[0] for f in engine.Rdm1Result._fields_] == ["ovlp", "abs_sum", "n_src", "n_terms", "n_hits"]
    assert engine.Rdm1._fields == ("gamma", "ovlp", "abs_sum", "n_src", "n_terms", "n_hits")
    for meth in ("expectation", "natural_occupations"):
        assert callable(getattr(engine.Rdm1, meth, None)), meth
    from fries_amd.replicas import FriReplicas
    assert callable(getattr(FriReplicas, "pair_rdm1", None))


def test_rdm1_derived_quantities_on_the_host():
    """Rdm1.expectation and Rdm1.natural_occupations are host arithmetic on the matrix: a closed-shell determinant's density matrix
    (2 on the occupied diagonal) gives n_elec and the occupations 2, 2, 0, 0; the overlap normalises."""
    import numpy as np
    import pytest
    g = np.diag([2.0, 2.0, 0.0, 0.0]) * 3.0
    r = engine.Rdm1(g, 3.0, 0.0, 1, 8, 0)
    assert r.expectation(np.eye(4)) == 4.0
    assert r.expectation(np.diag([1.0, 0.0, 5.0, 0.0])) == 2.0
    assert np.array_equal(r.natural_occupations(), [2.0, 2.0, 0.0, 0.0])
    with pytest.raises(ValueError):
        r.expectation(np.eye(3))
    skew = engine.Rdm1(np.array([[1.0, 4.0], [0.0, 1.0]]), 1.0, 4.0, 1, 2, 1)
    assert np.allclose(skew.natural_occupations(), [3.0, -1.0])           # (gamma + gamma.T) / 2 = [[1, 2], [2, 1]]
    assert np.array_equal(skew.transposed().gamma, [[1.0, 0.0], [4.0, 1.0]]) and skew.transposed()[1:] == skew[1:]


def _driver(*extra, env=None):
    assert os.path.exists(build.DRIVER), "frisys_mol_hip has not been built"
    cmd = [build.DRIVER, "--fcidump_path", os.path.join(ROOT, "no_such_dir", "no.FCIDUMP"), "--vec_nonz", "10", "--mat_nonz", "10", "--max_dets", "100",
           "--max_iter", "1", *extra]
    return subprocess.run(cmd, capture_output=True, text=True, timeout=60, env=env)


def test_driver_refuses_repl_rdm1_without_replicas():
    res = _driver("--repl_rdm1", "1", "--seed", "1")
    assert res.returncode != 0
    assert "--repl_rdm1 needs --replicas" in res.stderr, res.stderr
