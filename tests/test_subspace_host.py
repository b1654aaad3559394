"""No GPU: the host arithmetic of fries_amd/subspace.py (the inverse of the R factor, the generalised eigenvalues, adjust_shift2, the dense
model of the whole loop), the boundary of the four new entry points (library, header, Python layer), and the geometry of
csrc/axpy_plan.hpp replayed by a stand-alone program under AddressSanitizer and UBSan."""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

from fries_amd import engine, fcidump
from fries_amd import subspace as sp
from subspace_common import BURN_IN, MODEL_EPS, MODEL_RESTART, N_ITER, model_h

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("fries_vec_axpy_snapshot", "fries_snapshot_dot", "fries_vec_scale", "fries_vec_one_norm")


@pytest.mark.parametrize("n", [2, 3, 4, 5, 6])
def test_rinv_orthonormalises(n):
    rng = np.random.RandomState(100 + n)
    for _ in range(20):
        d, h = np.eye(n) + 0.3 * rng.standard_normal((n, n)), rng.standard_normal((n, n))
        m = d - 0.01 * h
        assert np.linalg.cond(m) < 100          # well-conditioned
        r_inv = sp.rinv(m)
        q = m @ r_inv
        assert np.abs(q.T @ q - np.eye(n)).max() <= 1e-12
        assert np.array_equal(r_inv, np.triu(r_inv))
        assert np.abs(np.abs(r_inv) - np.abs(np.linalg.inv(np.linalg.qr(m, mode="r")))).max() <= 1e-12


@pytest.mark.parametrize("n", [2, 3, 4, 5, 6])
def test_generalised_eigenvalues(n):
    rng = np.random.RandomState(200 + n)
    s = rng.standard_normal((n, n))
    s = (s + s.T) / 2                           # a symmetric problem seen through two bases: real eigenvalues
    t, x = np.eye(n) + 0.2 * rng.standard_normal((n, n)), np.eye(n) + 0.2 * rng.standard_normal((n, n))
    d, h = t.T @ x, t.T @ s @ x
    got = sp.gen_eigvals(d, h)
    assert np.all(np.diff(got) >= 0)
    # each is a root of det(H - lambda D): the smallest singular value of the pencil vanishes there, and only there
    for lam in got:
        sv = np.linalg.svd(h - lam * d, compute_uv=False)
        assert sv[-1] <= 1e-12 * sv[0] and (n == 1 or sv[-2] > 1e-6 * sv[0])
    # the issue's reference: numpy.linalg.eigvals(solve(D, H)), here through the transposed problem so that it is another computation
    want = np.sort(np.linalg.eigvals(np.linalg.solve(d.T, h.T).T).real)
    assert np.abs(got - want).max() <= 1e-10
    assert np.abs(got - np.linalg.eigvalsh(s)).max() <= 1e-10
    assert np.array_equal(sp.averaged_energies([d * 7, d, d], [h * 7, h, h], 1, offset=2.5), got + 2.5)


def test_adjust_shift2_is_the_references():
    # compress_utils.cpp:695-700 by hand: shift' = shift^(1 - d) (norm / last)^d, last' = last^d (norm / shift)^(1 - d)
    f, last = sp.adjust_shift2(1.0, 1000.0, 1000.0)
    assert (f, last) == (1.0, 1000.0)
    f, last = sp.adjust_shift2(1.21, 1440.0, 1000.0, 0.5)
    assert abs(f - 1.1 * 1.2) <= 1e-15 and abs(last - 1000.0 ** 0.5 * (1440.0 / 1.21) ** 0.5) <= 1e-12
    f, last = sp.adjust_shift2(2.0, 300.0, 100.0, 0.25)
    assert abs(f - 2.0 ** 0.75 * 3.0 ** 0.25) <= 1e-15 and abs(last - 100.0 ** 0.25 * 150.0 ** 0.75) <= 1e-12
    assert (sp.SHIFT_DAMPING, sp.SHIFT_INTERVAL) == (0.5, 1)


def test_dense_model_converges_to_the_three_lowest():
    h, trials = model_h()
    want = np.linalg.eigvalsh(h)[:3]
    rec = []
    d_mats, h_mats = sp.dense_model(h, trials, N_ITER, epsilon=MODEL_EPS, restart_int=MODEL_RESTART, record=rec)
    assert d_mats.shape == h_mats.shape == (N_ITER, 3, 3) and len(rec) == N_ITER // MODEL_RESTART
    got = sp.averaged_energies(d_mats, h_mats, BURN_IN)
    print("the model's error after", N_ITER, "iterations:", np.abs(got - want).max())
    assert np.abs(got - want).max() <= 1e-9
    short = sp.averaged_energies(*[m[:100] for m in (d_mats, h_mats)], 95)
    assert np.abs(short - want).max() > 1e-6        # (it is the iteration that gets there, not the trial vectors)
    # a restart orthonormalises what the trial vectors see: (D - eps H) R^-1 has orthonormal columns
    it, m, r_inv, before, after = rec[-1]
    q = m @ r_inv
    assert it == N_ITER - 1 and np.abs(q.T @ q - np.eye(3)).max() <= 1e-12
    # the extended-precision run the device tests measure the loop's rounding sensitivity with
    dl, hl = sp.dense_model(h, trials, N_ITER, epsilon=MODEL_EPS, restart_int=MODEL_RESTART, dtype=np.longdouble)
    rho = max(float(np.abs(d_mats[k] - dl[k]).max() / np.abs(dl[k]).max()) for k in range(N_ITER))
    print("largest relative difference of d_mats between float64 and longdouble:", rho)
    assert rho < 1e-9


def test_subspace_refuses_ranks_and_empty_input_before_any_engine():
    par = dict(epsilon=0.01, vec_nonz=10, mat_nonz=10, max_dets=100, restart_int=5)
    with pytest.raises(TypeError, match="ranks"):           # one rank per state: there is no such argument
        sp.FriSubspace(None, [(np.zeros(1, dtype=np.uint64), np.ones(1))], ranks=2, **par)
    with pytest.raises(ValueError, match="trial"):
        sp.FriSubspace(None, [], **par)
    with pytest.raises(ValueError, match="restart_int"):
        sp.FriSubspace(None, [(np.zeros(1, dtype=np.uint64), np.ones(1))], **dict(par, restart_int=0))
    sig = inspect.signature(sp.FriSubspace.__init__).parameters
    assert list(sig)[:3] == ["self", "mol", "trials"] and all(sig[k].kind is inspect.Parameter.KEYWORD_ONLY for k in ("epsilon", "vec_nonz", "mat_nonz", "max_dets", "restart_int"))
    assert (sig["initiator"].default, sig["seed"].default, sig["device"].default) == (0.0, 0, 0) and list(sig)[-1] == "device"
    for meth in ("iterate", "energies", "close", "trials_from_dets"):
        assert callable(getattr(sp.FriSubspace, meth))


def test_min6_shape():
    mol = fcidump.synthetic("MIN6")
    assert (mol.n_orb, mol.n_elec, mol.point_group) == (6, 4, "Cs") and list(mol.irreps) == [0, 1, 0, 1, 0, 1]
    from math import comb
    assert comb(6, 2) ** 2 == 225


# ------------------------------------------------------------------ the boundary
def test_library_exports_the_four_entry_points():
    assert os.path.exists(engine.LIB_PATH), "libfries_hip.so has not been built"
    lib = ctypes.CDLL(engine.LIB_PATH)
    for name in ENTRY_POINTS:
        assert hasattr(lib, name), name


def test_header_declares_them():
    with open(os.path.join(ROOT, "include", "fries_hip.h")) as f:
        header = f.read()
    decls = {
        "fries_vec_axpy_snapshot": r"fries_ctx\s*\*\s*ctx\s*,\s*int\s+column\s*,\s*double\s+coeff\s*,\s*const\s+fries_snapshot\s*\*\s*x\s*,\s*uint64_t\s*\*\s*n_taken",
        "fries_snapshot_dot": r"fries_ctx\s*\*\s*const\s*\*\s*a\s*,\s*uint32_t\s+n_a\s*,\s*int\s+column\s*,\s*const\s+fries_snapshot\s*\*\s*b\s*,\s*fries_vdot_result\s*\*\s*out",
        "fries_vec_scale": r"fries_ctx\s*\*\s*ctx\s*,\s*int\s+column\s*,\s*double\s+factor",
        "fries_vec_one_norm": r"fries_ctx\s*\*\s*ctx\s*,\s*int\s+column\s*,\s*double\s*\*\s*norm",
    }
    assert set(decls) == set(ENTRY_POINTS)
    for name, args in decls.items():
        assert re.search(r"\bint\s+" + name + r"\s*\(\s*" + args + r"\s*\)\s*;", header), name
    m = re.search(r"typedef\s+struct\s*\{([^}]*)\}\s*fries_vdot_result\s*;", header)
    assert m and " ".join(m.group(1).split()) == "double dot, abs_sum; uint64_t n_src, n_hits;"


def test_python_layer_lists_and_wraps_them():
    for name in ENTRY_POINTS:
        assert name in engine.EXPORTS, name
    assert ctypes.sizeof(engine.VdotResult) == 32 and [f[0] for f in engine.VdotResult._fields_] == ["dot", "abs_sum", "n_src", "n_hits"]
    assert engine.VDot._fields == ("dot", "abs_sum", "n_src", "n_hits")
    eng = engine.FriEngine
    assert list(inspect.signature(eng.axpy_snapshot).parameters) == ["self", "column", "coeff", "snap"]
    assert list(inspect.signature(eng.scale).parameters) == ["self", "column", "factor"]
    assert inspect.signature(eng.one_norm).parameters["column"].default == 0
    assert inspect.signature(engine.VecSnapshot.dot).parameters["column"].default == 0


def test_axpy_plan_replay_under_sanitizers(tmp_path):
    """tests/cpp/axpy_plan_check.cpp, host only: g++ -fsanitize=address,undefined, its own main, nothing loaded into Python (the
    sanitizers' runtimes are linked statically).  Its cases: 0 entries, 1 entry, a tile edge (1024, 1025), the capacity exactly, the
    capacity plus one, a rank that owns nothing."""
    exe = str(tmp_path / "axpy_plan_check")
    src = os.path.join(ROOT, "tests", "cpp", "axpy_plan_check.cpp")
    res = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-o", exe, src], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr[-3000:]
    res = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(res.stdout[-2000:])
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-3000:]
    assert re.search(r"\b\d+ geometries, 0 failures\b", res.stdout)
