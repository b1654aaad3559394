"""The two-body density matrix between replicas as a boundary, checked without a GPU: libfries_hip.so exports fries_rdm2, include/fries_hip.h
declares it and its result struct, the Python layer lists and wraps it, FriReplicas has pair_rdm2, Rdm2's methods are host arithmetic,
frisys_mol_hip refuses --repl_rdm2 without --replicas before it touches a device, and the chunk cutting and scratch layout of
csrc/rdm2_plan.hpp pass a stand-alone replay under AddressSanitizer and UBSan."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from fries_amd import build, engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_fries_rdm2():
    assert os.path.exists(engine.LIB_PATH), "libfries_hip.so has not been built"
    assert hasattr(ctypes.CDLL(engine.LIB_PATH), "fries_rdm2")


def test_header_declares_the_call_and_its_result():
    with open(os.path.join(ROOT, "include", "fries_hip.h")) as f:
        header = f.read()
    assert re.search(r"\bint\s+fries_rdm2\s*\(\s*fries_ctx\s*\*\s*a\s*,\s*fries_ctx\s*\*\s*b\s*,\s*double\s*\*\s*gamma2\s*(/\*.*?\*/)?\s*,\s*fries_rdm2_result\s*\*\s*out\s*\)\s*;", header)
    m = re.search(r"typedef\s+struct\s*\{([^}]*)\}\s*fries_rdm2_result\s*;", header)
    assert m, "struct fries_rdm2_result is not declared"
    body = " ".join(m.group(1).split())
    assert body == "double ovlp, abs_sum; uint64_t n_src, n_terms, n_hits;", body
    # the header comment states the definition, the identities, the threading contract, determinism, the refusals and what is out of scope
    for phrase in ("c+_{p sigma} c+_{r tau} c_{s tau} c_{q sigma}", "chemists' order", "(n_elec - 1) gamma[p][q]", "bit for bit", "<S^2>",
                   "on another thread", "no floating-point atomics", "FRIES_RDM2_RECORDS", "spin_parity != 0", "hf_en is not compared", "three-body"):
        assert phrase in header, phrase


def test_python_layer_lists_and_wraps_it():
    assert "fries_rdm2" in engine.EXPORTS
    assert callable(getattr(engine.FriEngine, "rdm2", None))
    assert ctypes.sizeof(engine.Rdm2Result) == 40
    assert [f[0] for f in engine.Rdm2Result._fields_] == ["ovlp", "abs_sum", "n_src", "n_terms", "n_hits"]
    assert engine.Rdm2._fields == ("gamma2", "ovlp", "abs_sum", "n_src", "n_terms", "n_hits")
    for meth in ("transposed", "partial_trace", "expectation", "energy", "spin_squared"):
        assert callable(getattr(engine.Rdm2, meth, None)), meth
    from fries_amd.replicas import FriReplicas
    assert callable(getattr(FriReplicas, "pair_rdm2", None))


def _closed_shell(n_orb, n_docc, ovlp):
    """Gamma of one determinant with orbitals 0 .. n_docc - 1 doubly occupied, times ovlp: every ordered pair of occupied spin orbitals
    gives +1 to [p,p,r,r] and, with equal spins, -1 to [p,r,r,p]"""
    g = np.zeros((n_orb,) * 4)
    so = [(p, s) for s in (0, 1) for p in range(n_docc)]
    for (p, sp) in so:
        for (r, sr) in so:
            if (p, sp) == (r, sr):
                continue
            g[p, p, r, r] += ovlp
            if sp == sr:
                g[p, r, r, p] -= ovlp
    return g


def test_rdm2_derived_quantities_on_the_host():
    n, n_docc, n_elec = 4, 2, 4
    r = engine.Rdm2(_closed_shell(n, n_docc, 3.0), 3.0, 0.0, 1, 0, 0)
    assert r.spin_squared(n_elec) == 0.0
    # the partial trace is the one-body density matrix: 2 on the occupied diagonal, times the overlap
    want = np.diag([2.0, 2.0, 0.0, 0.0]) * 3.0
    assert np.array_equal(r.partial_trace(n_elec), want)
    assert np.array_equal(r.partial_trace(n_elec), np.einsum("pqrr->pq", r.gamma2) / (n_elec - 1))
    unit = np.einsum("pq,rs->pqrs", np.eye(n), np.eye(n))
    assert r.expectation(unit) == n_elec * (n_elec - 1) / 2
    # energy: with h = identity and eri4 = the unit operator, n_elec + n_elec (n_elec - 1) / 2
    assert r.energy(np.eye(n), unit, want) == n_elec + n_elec * (n_elec - 1) / 2
    for bad in (np.zeros((n,) * 3), np.zeros((n + 1,) * 4), np.eye(n)):
        with pytest.raises(ValueError):
            r.expectation(bad)
    with pytest.raises(ValueError):
        r.energy(np.eye(n + 1), unit, want)
    # the adjoint view: [p, q, r, s] -> [q, p, s, r], everything else as it is
    g = np.arange(16.0).reshape(2, 2, 2, 2)
    t = engine.Rdm2(g, 1.0, 2.0, 3, 4, 5).transposed()
    assert t[1:] == (1.0, 2.0, 3, 4, 5) and t.gamma2.flags["C_CONTIGUOUS"]
    for p, q, rr, s in np.ndindex(2, 2, 2, 2):
        assert t.gamma2[p, q, rr, s] == g[q, p, s, rr]
    # a triplet: |0 alpha 1 alpha> has S = 1, <S^2> = 2
    trip = np.zeros((2,) * 4)
    for p, rr in ((0, 1), (1, 0)):
        trip[p, p, rr, rr] += 1.0
        trip[p, rr, rr, p] -= 1.0
    assert engine.Rdm2(trip, 1.0, 0.0, 1, 0, 0).spin_squared(2) == 2.0


def _driver(*extra):
    assert os.path.exists(build.DRIVER), "frisys_mol_hip has not been built"
    cmd = [build.DRIVER, "--fcidump_path", os.path.join(ROOT, "no_such_dir", "no.FCIDUMP"), "--vec_nonz", "10", "--mat_nonz", "10", "--max_dets", "100",
           "--max_iter", "1", *extra]
    return subprocess.run(cmd, capture_output=True, text=True, timeout=60)


def test_driver_refuses_repl_rdm2_without_replicas():
    res = _driver("--repl_rdm2", "1", "--seed", "1")
    assert res.returncode != 0
    assert "--repl_rdm2 needs --replicas" in res.stderr, res.stderr


def test_plan_replay_under_sanitizers(tmp_path):
    """tests/cpp/rdm2_plan_check.cpp, host only: g++ -fsanitize=address,undefined, its own main, nothing loaded into Python (the
    sanitizers' runtimes are linked statically, so that the program starts whatever else the loader brings in)"""
    exe = str(tmp_path / "rdm2_plan_check")
    src = os.path.join(ROOT, "tests", "cpp", "rdm2_plan_check.cpp")
    res = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-o", exe, src], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr[-3000:]
    res = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(res.stdout[-2000:])
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-3000:]
    assert re.search(r"\b\d+ geometries, 0 failures\b", res.stdout)
