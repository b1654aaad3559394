"""-m gpu: the replica estimator fries_h_dot (csrc/hdot.hip) and the replica runs built on it.

The reference of every numerical check is formed here, on the host: the dense matrix column by column from fries_h_offdiag_list (one
source, value 1: the elements as k_enum generates them), the diagonal from fries_matrel_batch minus the run's offset, and the sums with
math.fsum.  With u = 2**-53, N non-zero terms and abs_ref the fsum of their magnitudes, a sum of N doubles in ANY order is within
(N - 1) u abs_ref of the exact one, the two roundings of every product a_i * m * b_j add 2 u abs_ref on either side and fsum one more:
(N + 8) u abs_ref bounds the difference whatever tree the device uses.  It is a worst case, not a measured tolerance."""
import math
import os
import subprocess

import numpy as np
import pytest

import golden_io
import pair_common as pc
from fries_amd import fcidump
from pair_common import SMALL, U, as_map as _as_map, ne_run as _ne_run

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def Engine():
    from fries_amd.engine import FriEngine
    return FriEngine


# ------------------------------------------------------------------ the host reference
def _dense(eng, dets):
    """H on `dets` as the device generates it: cols[i] = {j: <j|H|i>} (off-diagonal, non-zero) and diag[i] = <i|H|i> - offset."""
    dets = np.asarray(sorted(int(d) for d in dets), dtype=np.uint64)
    cols = {}
    for d in dets:
        od, ov = eng.h_offdiag_list(np.array([d], dtype=np.uint64), np.ones(1))
        cols[int(d)] = {int(t): float(x) for t, x in zip(od, ov) if x != 0.0 and int(t) != int(d)}
    dg = eng.matrel(0, dets)[0] - eng.hf_energy
    return cols, {int(d): float(x) for d, x in zip(dets, dg)}


def _reference(a, b, cols, diag):
    """what fries_h_dot(a, b) sums, term by term (a enumerates, b is probed)"""
    h_terms, ov_terms = [], []
    n_src = n_terms = n_hits = 0
    for i, ai in a.items():
        n_src += 1
        bi = b.get(i, 0.0)
        if bi != 0.0:
            ov_terms.append(ai * bi)
            h_terms.append(ai * diag[i] * bi)
        for j, m in cols[i].items():
            n_terms += 1
            bj = b.get(j, 0.0)
            if bj != 0.0:
                n_hits += 1
                h_terms.append(ai * m * bj)
    h_terms = [t for t in h_terms if t != 0.0]
    return dict(h=math.fsum(h_terms), abs_h=math.fsum(abs(t) for t in h_terms), n_h=len(h_terms), ovlp=math.fsum(ov_terms),
                abs_ov=math.fsum(abs(t) for t in ov_terms), n_ov=len(ov_terms), n_src=n_src, n_terms=n_terms, n_hits=n_hits)


def _check(tag, res, ref):
    bound_h, bound_ov = (ref["n_h"] + 8) * U * ref["abs_h"], (ref["n_ov"] + 8) * U * ref["abs_ov"]
    print(f"{tag}: n_src {res.n_src} n_terms {res.n_terms} n_hits {res.n_hits}; h {res.h!r} ref {ref['h']!r} err {abs(res.h - ref['h']):.3e} bound {bound_h:.3e}; "
          f"ovlp {res.ovlp!r} err {abs(res.ovlp - ref['ovlp']):.3e} bound {bound_ov:.3e}; abs_sum {res.abs_sum!r} err {abs(res.abs_sum - ref['abs_h']):.3e}")
    assert (res.n_src, res.n_terms, res.n_hits) == (ref["n_src"], ref["n_terms"], ref["n_hits"]), tag
    assert abs(res.h - ref["h"]) <= bound_h, tag
    assert abs(res.abs_sum - ref["abs_h"]) <= bound_h, tag
    assert abs(res.ovlp - ref["ovlp"]) <= bound_ov, tag
    return bound_h


def _check_all(ea, eb, a, b, cols, diag):
    """(a, b), (b, a) and (a, a) against the dense matrix, the symmetry of the estimate, and bit-identical repeats"""
    r_ab, r_ba, r_aa = ea.h_dot(eb), eb.h_dot(ea), ea.h_dot()
    bound = _check("(a,b)", r_ab, _reference(a, b, cols, diag))
    _check("(b,a)", r_ba, _reference(b, a, cols, diag))
    _check("(a,a)", r_aa, _reference(a, a, cols, diag))
    assert abs(r_ab.h - r_ba.h) <= bound and abs(r_ab.abs_sum - r_ba.abs_sum) <= bound      # H is symmetric
    assert r_aa.ovlp > 0 and ea.variational_energy() == r_aa.h / r_aa.ovlp
    assert ea.h_dot(ea) == r_aa
    for _ in range(3):
        assert ea.h_dot(eb) == r_ab and eb.h_dot(ea) == r_ba       # NamedTuple equality of floats: the same bits (no NaN, no signed zero at stake)
    return r_ab


# ------------------------------------------------------------------ 1. whole space
def test_whole_space_min4(Engine, mols):
    """2 electrons in 4 orbitals, C1: all 16 determinants in both vectors, in different orders, two exact zeros each."""
    mol = mols("MIN4")
    ea, eb, dets, (da, va), (db, vb) = pc.min4_pair(Engine, mol, 20251)
    eh = Engine(mol)
    eh.setup(epsilon=0.01, vec_nonz=50, mat_nonz=50, max_dets=1000, seed=3, distribution="HB_unnorm")
    cols, diag = _dense(eh, dets)
    assert sum(len(c) for c in cols.values()) > 100         # (one irrep: nearly every pair of determinants is connected)
    res = _check_all(ea, eb, _as_map(da, va), _as_map(db, vb), cols, diag)
    assert res.n_src == 14
    for e in (ea, eb, eh):
        e.close()


# ------------------------------------------------------------------ 2. compressed vectors of two runs
def test_sparse_vectors_with_symmetry_misses_and_holes(Engine, mols):
    """Two Ne runs (seeds 1 and 2), 25 iterations at vec_nonz = mat_nonz = 150: compressed vectors with released positions and a hash
    table that has seen deletions; D2h, so most candidate slots are rejected by symmetry and most targets are not in the other vector."""
    mol = mols("Ne")
    ea, eb = pc.ne_pair(Engine, mol)
    eh = Engine(mol)
    eh.setup(**SMALL)
    (da, va), (db, vb) = ea.vector(), eb.vector()
    a, b = _as_map(da, va), _as_map(db, vb)
    assert len(a) < da.size or len(b) < db.size or ea.vec_info()[2] + eb.vec_info()[2] > 0, "no released position in either vector"
    cols, diag = _dense(eh, set(a) | set(b))
    res = _check_all(ea, eb, a, b, cols, diag)
    assert 0 < res.n_hits < res.n_terms          # seeds (1, 2): hits and misses both occur
    for e in (ea, eb, eh):
        e.close()


# ------------------------------------------------------------------ 3. time reversal
@pytest.mark.parametrize("spin_parity", [1, -1])
def test_time_reversal(Engine, mols, spin_parity):
    """Vectors of representatives (what one fries_h_offdiag_list call on the tr_ne fixture's input returns), elements between the
    symmetrised functions.  Reference: a . (H_offdiag b) from fries_h_offdiag_list on b, plus the diagonal.  No count assertions: two
    excitations can share a target under time reversal.  The bound uses the device's own abs_sum, which the tests above validate."""
    mol = mols("Ne")
    sd, sv, _ = golden_io.read_tr("tr_ne")
    ea, eb, eh = Engine(mol), Engine(mol), Engine(mol)
    for e in (ea, eb, eh):
        e.setup(**SMALL)
        e.set_spin_parity(spin_parity)
    reps, _ = eh.h_offdiag_list(sd, sv)
    reps = np.unique(reps)
    rng = np.random.RandomState(77 + spin_parity)
    da, db = reps[rng.rand(reps.size) < 0.6], reps[rng.rand(reps.size) < 0.6]
    da, db = da[:300], db[:300]         # (a few hundred sources keep the reference call short)
    va, vb = rng.standard_normal(da.size), rng.standard_normal(db.size)
    assert da.size > 50 and db.size > 50 and np.intersect1d(da, db).size > 10
    ea.vec_load(da, va)
    eb.vec_load(db, vb)
    a = _as_map(da, va)
    for (ex, ey, x, dy, vy, tag) in ((ea, eb, a, db, vb, "(a,b)"), (eb, ea, _as_map(db, vb), da, va, "(b,a)")):
        hd, hv = eh.h_offdiag_list(dy, vy)
        hy = _as_map(hd, hv)
        y = _as_map(dy, vy)
        common = np.array(sorted(set(x) & set(y)), dtype=np.uint64)
        dg = eh.matrel(0, common)[0] - eh.hf_energy
        terms = [x[i] * hy[i] for i in x if i in hy] + [x[int(i)] * float(d) * y[int(i)] for i, d in zip(common, dg)]
        ref = math.fsum(terms)
        res = ex.h_dot(ey)
        bound = (res.n_terms + res.n_src + 8) * U * res.abs_sum
        print(f"spin parity {spin_parity} {tag}: h {res.h!r} ref {ref!r} err {abs(res.h - ref):.3e} bound {bound:.3e} n_terms {res.n_terms} n_hits {res.n_hits}")
        assert res.n_hits > 0 and res.abs_sum > 0
        assert abs(res.h - ref) <= bound, tag
        assert ex.h_dot(ey) == res
    for e in (ea, eb, eh):
        e.close()


# ------------------------------------------------------------------ 4. refusals
def _h_dot(a, b):
    return a.h_dot(b)


def _refused(a, b, match):
    pc.refused(_h_dot, "fries_h_dot", a, b, match)


def test_refusals_launch_nothing(Engine, mols):
    from fries_amd.engine import HdotResult
    mol = mols("Ne")
    plain = Engine(mol)
    plain.setup(**SMALL)
    pc.check_common_refusals(Engine, mols, plain, _h_dot, "fries_h_dot", HdotResult)
    # the same shape with other integrals: hf_en, the offset of the diagonal, differs
    other = Engine(fcidump.synthetic("Ne", seed=777))
    other.setup(**SMALL)
    _refused(plain, other, "different molecules")
    _refused(other, plain, "different molecules")
    other.close()
    # different spin parity
    flipped = Engine(mol)
    flipped.setup(**SMALL)
    flipped.set_spin_parity(1)
    _refused(plain, flipped, "spin_parity")
    flipped.set_spin_parity(0)
    assert plain.h_dot(flipped) == plain.h_dot()        # two engines with the same set-up hold the same vector
    flipped.close()
    plain.close()


# ------------------------------------------------------------------ 5. the estimator reads, and only reads
def test_estimator_does_not_disturb_the_run(Engine, mols):
    mol = mols("Ne")
    par = _ne_run()
    quiet, probed = Engine(mol), Engine(mol)
    quiet.setup(**par)
    probed.setup(**par)
    lq, lp = [], []
    for _ in range(20):
        lq.append(quiet.iterate(1))
        lp.append(probed.iterate(1))
        s, o = probed.h_dot(), probed.h_dot(quiet)
        assert s == o and s.n_hits > 0          # the two engines hold the same vector
    pc.assert_same_run(quiet, probed, np.concatenate(lq), np.concatenate(lp))
    quiet.close()
    probed.close()


def test_estimator_returns_its_device_memory(Engine, mols):
    pc.check_device_memory_returned(Engine, mols("Ne"), _h_dot, "fries_h_dot")


# ------------------------------------------------------------------ 6. FriReplicas
def test_replicas_equal_lone_engines(Engine, mols):
    from fries_amd.replicas import FriReplicas
    mol = mols("Ne")
    par = _ne_run()
    seed = par.pop("seed")
    reps = FriReplicas(mol, 3, seed, **par)
    logs = reps.iterate(20)
    assert len(logs) == 3 and len(reps.engines) == 3
    for r in range(3):
        lone = Engine(mol)
        lone.setup(seed=seed + r, **par)
        want = lone.iterate(20)
        assert logs[r].tobytes() == want.tobytes(), r
        (dl, vl), (dr, vr) = lone.vector(), reps.engines[r].vector()
        assert vl.tobytes() == vr.tobytes() and dl.tobytes() == dr.tobytes(), r
        lone.close()
    assert logs[0].tobytes() != logs[1].tobytes()       # different seeds: different trajectories
    est = reps.pair_estimates()
    assert len(est) == 3 and reps.pairs() == [(0, 1), (0, 2), (1, 2)]
    nz = [e.vec_info()[1] for e in reps.engines]
    for (r, s), got in zip(reps.pairs(), est):
        a, b = (r, s) if nz[r] <= nz[s] else (s, r)
        assert got == reps.engines[a].h_dot(reps.engines[b]), (r, s)
        assert got.n_hits > 0 and got.ovlp != 0
        print(f"pair ({r},{s}): h / ovlp = {got.h / got.ovlp!r}")
    reps.close()
    assert reps.engines == []


# ------------------------------------------------------------------ 7. the command line
def _lines(path):
    with open(path) as f:
        return f.read().split()


def test_a_failing_replica_releases_the_others(mols, tmp_path):
    """Replica 1 cannot open its output files (its directory's name is taken by a regular file) and throws after its set-up; replica 0
    runs on to the first meeting point, is sent home from the barrier, and the process returns non-zero instead of waiting."""
    from fries_amd import build
    mol = mols("Ne")
    fc = str(tmp_path / "mol.FCIDUMP")
    fcidump.write_fcidump(fc, mol)
    out = str(tmp_path / "run") + "/"
    os.makedirs(out)
    with open(out + "replica1", "w") as f:
        f.write("in the way\n")
    res = subprocess.run(pc.cmd(build.DRIVER, fc, mol, _ne_run(), 10, out, 5) + ["--replicas", "2", "--repl_every", "5"], capture_output=True, text=True, timeout=300)
    assert res.returncode != 0
    assert "Exception on replica 1" in res.stderr and "Could not" in res.stderr, res.stderr[-2000:]
    assert "Exception on replica 0 : another replica failed" in res.stderr, res.stderr[-2000:]
    assert _lines(out + "repliter.txt") == []


def test_command_line_replicas(Engine, mols, tmp_path):
    from fries_amd import build
    mol = mols("Ne")
    par = _ne_run()
    seed = 20250215
    fc = str(tmp_path / "mol.FCIDUMP")
    fcidump.write_fcidump(fc, mol)
    dirs = {k: str(tmp_path / k) + "/" for k in ("repl", "plain0", "plain1", "one")}
    for d in dirs.values():
        os.makedirs(d)
    pc.run(pc.cmd(build.DRIVER, fc, mol, par, 30, dirs["repl"], seed) + ["--replicas", "2", "--repl_every", "10"])
    pc.run(pc.cmd(build.DRIVER, fc, mol, par, 30, dirs["plain0"], seed))
    pc.run(pc.cmd(build.DRIVER, fc, mol, par, 30, dirs["plain1"], seed + 1))
    for r in range(2):
        rd, pd = dirs["repl"] + f"replica{r}/", dirs[f"plain{r}"]
        names = sorted(os.listdir(pd))
        assert sorted(os.listdir(rd)) == names and "projnum.txt" in names and "dets0.dat" in names
        for n in names:
            with open(rd + n, "rb") as f, open(pd + n, "rb") as g:
                assert f.read() == g.read(), (r, n)
    assert _lines(dirs["repl"] + "repliter.txt") == ["10", "20", "30"]
    num, den = _lines(dirs["repl"] + "replnum.txt"), _lines(dirs["repl"] + "replden.txt")
    assert len(num) == 3 and len(den) == 3 and all("," not in x for x in num + den)
    # the last line against fries_h_dot on the two final checkpoints (positions differ after a load, so the bits may)
    engs = []
    for r in range(2):
        e = Engine(mol)
        e.setup(**dict(par, seed=seed + r))
        e.vec_load(*pc.saved_vector(dirs["repl"] + f"replica{r}/", mol))
        engs.append(e)
    a, b = (0, 1) if engs[0].vec_info()[1] <= engs[1].vec_info()[1] else (1, 0)
    res = engs[a].h_dot(engs[b])
    bound = (res.n_hits + res.n_src + 8) * U * res.abs_sum
    print(f"replnum {num[-1]} h_dot {res.h!r} err {abs(float(num[-1]) - res.h):.3e}; replden {den[-1]} ovlp {res.ovlp!r} err {abs(float(den[-1]) - res.ovlp):.3e}; bound {bound:.3e}")
    assert abs(float(num[-1]) - res.h) <= bound
    assert abs(float(den[-1]) - res.ovlp) <= bound
    # one replica: the pair (0, 0), the Rayleigh quotient of the vector
    pc.run(pc.cmd(build.DRIVER, fc, mol, par, 30, dirs["one"], seed) + ["--replicas", "1", "--repl_every", "10"])
    assert _lines(dirs["one"] + "repliter.txt") == ["10", "20", "30"]
    num1, den1 = _lines(dirs["one"] + "replnum.txt"), _lines(dirs["one"] + "replden.txt")
    assert len(num1) == 3 and len(den1) == 3 and all("," not in x for x in num1 + den1)
    with open(dirs["one"] + "replica0/vals0.dat", "rb") as f, open(dirs["plain0"] + "vals0.dat", "rb") as g:
        assert f.read() == g.read()
    self0 = engs[0].h_dot()
    bound0 = (self0.n_hits + self0.n_src + 8) * U * self0.abs_sum
    assert abs(float(num1[-1]) - self0.h) <= bound0 and abs(float(den1[-1]) - self0.ovlp) <= bound0
    assert float(den1[-1]) > 0
    for e in engs:
        e.close()
