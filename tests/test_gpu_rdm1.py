"""-m gpu: the one-body density matrix between replicas, fries_rdm1 (csrc/rdm1.hip), and what is built on it.

The reference of every numerical check is formed here from the definition, over Python integers and independent of the device code:
for every non-zero a_i, each spin, each occupied p and each empty q, the two bits are flipped, the occupied bits strictly between them
counted, and the result looked up in a dict of b; the terms are collected per bin and summed with math.fsum, the diagonal added as
a_i b_i per occupied spin orbital.  With u = 2**-53 every term is one rounded product, and a sum of n doubles in ANY order is within
(n - 1) u S of the exact one (S = the sum of the magnitudes): |device - reference| <= (n + 8) u S per bin, whatever order the device
adds in; the 8 covers the products and fsum's own rounding.  ovlp and abs_sum are bounded the same way.  Worst cases, not measured."""
import dataclasses
import math
import os

import numpy as np
import pytest

import pair_common as pc
from fries_amd import fcidump
from pair_common import SMALL, U, as_map as _as_map, ne_run as _ne_run, same_bits as _same_bits

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the geometry of csrc/rdm1_plan.hpp: positions per workgroup, partial matrices one workgroup of the fold adds
RD_BPOS, RD_FAN = 256, 64


@pytest.fixture(scope="module")
def Engine():
    from fries_amd.engine import FriEngine
    return FriEngine


# ------------------------------------------------------------------ the host reference
def _reference(a, b, n_orb):
    """gamma(a, b) term by term (a enumerates, b is looked up): per bin the fsum, the sum of magnitudes and the number of terms"""
    terms = {}
    ov_terms = []
    n_src = n_terms = n_hits = 0
    orbs = range(n_orb)
    get = b.get
    for i, ai in a.items():
        n_src += 1
        for spin in (0, 1):
            sh = spin * n_orb
            occ = [p for p in orbs if (i >> (p + sh)) & 1]
            emp = [q for q in orbs if not (i >> (q + sh)) & 1]
            n_terms += len(occ) * len(emp)
            for p in occ:
                ip = i ^ (1 << (p + sh))
                for q in emp:
                    bj = get(ip ^ (1 << (q + sh)))
                    if bj is None:
                        continue
                    lo, hi = (p, q) if p < q else (q, p)
                    between = bin((i >> (lo + sh + 1)) & ((1 << (hi - lo - 1)) - 1)).count("1")
                    n_hits += 1
                    terms.setdefault((p, q), []).append(ai * (-1 if between & 1 else 1) * bj)
        bi = get(i)
        if bi is not None:
            t = ai * bi
            ov_terms.append(t)
            for P in range(2 * n_orb):
                if (i >> P) & 1:
                    terms.setdefault((P % n_orb, P % n_orb), []).append(t)
    gamma, mag, cnt = np.zeros((n_orb, n_orb)), np.zeros((n_orb, n_orb)), np.zeros((n_orb, n_orb), dtype=np.int64)
    for (p, q), ts in terms.items():
        gamma[p, q], mag[p, q], cnt[p, q] = math.fsum(ts), math.fsum(abs(t) for t in ts), len(ts)
    off = [abs(t) for (p, q), ts in terms.items() if p != q for t in ts]
    return dict(gamma=gamma, bound=(cnt + 8) * U * mag, cnt=cnt, ovlp=math.fsum(ov_terms), bound_ov=(len(ov_terms) + 8) * U * math.fsum(abs(t) for t in ov_terms),
                abs_sum=math.fsum(off), bound_abs=(len(off) + 8) * U * math.fsum(off), n_src=n_src, n_terms=n_terms, n_hits=n_hits)


def _check_gamma(tag, gamma, ref, transposed=False):
    want, bound = (ref["gamma"].T, ref["bound"].T) if transposed else (ref["gamma"], ref["bound"])
    err = np.abs(gamma - want)
    worst = np.unravel_index(np.argmax(err - bound), err.shape)
    print(f"{tag}: {int((want != 0).sum())} non-zero bins; worst bin {worst}: device {gamma[worst]!r} reference {want[worst]!r} err {err[worst]:.3e} bound {bound[worst]:.3e}")
    assert gamma.shape == want.shape
    assert np.all(err <= bound), tag


def _check(tag, res, ref):
    print(f"{tag}: n_src {res.n_src} n_terms {res.n_terms} n_hits {res.n_hits}; ovlp {res.ovlp!r} err {abs(res.ovlp - ref['ovlp']):.3e} bound {ref['bound_ov']:.3e}; "
          f"abs_sum {res.abs_sum!r} err {abs(res.abs_sum - ref['abs_sum']):.3e} bound {ref['bound_abs']:.3e}")
    assert (res.n_src, res.n_terms, res.n_hits) == (ref["n_src"], ref["n_terms"], ref["n_hits"]), tag
    _check_gamma(tag, res.gamma, ref)
    assert abs(res.ovlp - ref["ovlp"]) <= ref["bound_ov"], tag
    assert abs(res.abs_sum - ref["abs_sum"]) <= ref["bound_abs"], tag


def _check_trace(tag, res, ref, n_elec):
    tr, bound = float(np.trace(res.gamma)), float(np.trace(ref["bound"])) + n_elec * ref["bound_ov"] + 2 * n_elec * U * abs(n_elec * ref["ovlp"])
    print(f"{tag}: trace {tr!r} n_elec * ovlp {n_elec * res.ovlp!r} bound {bound:.3e}")
    assert abs(tr - n_elec * res.ovlp) <= bound, tag     # (the last term: np.trace's own additions)


# ------------------------------------------------------------------ 1. whole space
def test_whole_space_min4(Engine, mols):
    """2 electrons in 4 orbitals, C1: all 16 determinants in both vectors, in different orders, two exact zeros each (the construction of
    test_gpu_hdot.py::test_whole_space_min4)."""
    mol = mols("MIN4")
    ea, eb, _, (da, va), (db, vb) = pc.min4_pair(Engine, mol, 20251)
    a, b = _as_map(da, va), _as_map(db, vb)
    r_ab, r_ba, r_aa = ea.rdm1(eb), eb.rdm1(ea), ea.rdm1()
    ref_ab = _reference(a, b, mol.n_orb)
    _check("(a,b)", r_ab, ref_ab)
    _check("(b,a)", r_ba, _reference(b, a, mol.n_orb))
    _check("(a,a)", r_aa, _reference(a, a, mol.n_orb))
    assert r_ab.gamma.shape == (4, 4) and r_ab.n_src == 14 and r_ab.n_terms == 14 * mol.n_elec * (mol.n_orb - mol.n_elec // 2)
    # gamma(a, b)[p][q] = gamma(b, a)[q][p]: the same products (a bin has at most 8 here) in another order, so 2 (n - 1) u S <= (n + 8) u S apart
    assert ref_ab["cnt"].max() <= 8 and np.all(np.abs(r_ab.gamma - r_ba.gamma.T) <= ref_ab["bound"])
    assert np.all(r_ab.gamma != 0) and np.all(ref_ab["gamma"] != 0)
    for tag, r, ref in (("(a,b)", r_ab, ref_ab), ("(a,a)", r_aa, _reference(a, a, mol.n_orb))):
        _check_trace(tag, r, ref, mol.n_elec)
    assert _same_bits(ea.rdm1(ea), r_aa)
    for _ in range(3):
        assert _same_bits(ea.rdm1(eb), r_ab) and _same_bits(eb.rdm1(ea), r_ba)
    for e in (ea, eb):
        e.close()


# ------------------------------------------------------------------ 2. compressed vectors with holes
def test_sparse_vectors_with_holes(Engine, mols):
    """Two Ne runs (seeds 1 and 2), 25 iterations at vec_nonz = mat_nonz = 150: compressed vectors with released positions and a hash
    table that has seen deletions; most targets are not in the other vector."""
    mol = mols("Ne")
    ea, eb = pc.ne_pair(Engine, mol)
    (da, va), (db, vb) = ea.vector(), eb.vector()
    a, b = _as_map(da, va), _as_map(db, vb)
    assert len(a) < da.size or len(b) < db.size or ea.vec_info()[2] + eb.vec_info()[2] > 0, "no released position in either vector"
    r_ab, r_ba = ea.rdm1(eb), eb.rdm1(ea)
    ref = _reference(a, b, mol.n_orb)
    _check("(a,b)", r_ab, ref)
    _check("(b,a)", r_ba, _reference(b, a, mol.n_orb))
    _check("(a,a)", ea.rdm1(), _reference(a, a, mol.n_orb))
    _check_gamma("(b,a) transposed", r_ba.gamma.T, ref)
    _check_trace("(a,b)", r_ab, ref, mol.n_elec)
    assert 0 < r_ab.n_hits < r_ab.n_terms
    assert r_ab.n_terms == r_ab.n_src * mol.n_elec * (mol.n_orb - mol.n_elec // 2)
    off = ref["gamma"] - np.diag(np.diag(ref["gamma"]))
    print(f"{da.size} and {db.size} positions, {len(a)} and {len(b)} non-zero, {int((off != 0).sum())} non-zero off-diagonal bins")
    assert (off != 0).sum() > 0
    for _ in range(3):
        assert _same_bits(ea.rdm1(eb), r_ab)
    for e in (ea, eb):
        e.close()


# ------------------------------------------------------------------ 3. vectors that ignore symmetry
def test_vectors_that_ignore_symmetry(Engine, mols):
    """Ne shape, 600 determinants with n_elec / 2 electrons per spin from RandomState(7), loaded with vec_load: 100 random roots and
    five random same-spin single replacements of each, with no regard to the orbitals' irreps (random determinants alone are never
    one replacement apart: the space has 5e7 of them).  a and b take 75 % of the pool each, so they share about half of it; values
    are normal with a few exact zeros.  fries_rdm1 consults no symmetry table: bins whose orbitals differ in irrep are as good as any."""
    mol = mols("Ne")
    n, half = mol.n_orb, mol.n_elec // 2
    rng = np.random.RandomState(7)

    def string():
        return sum(1 << int(p) for p in rng.choice(n, half, replace=False))

    pool = []
    while len(pool) < 600:
        root = string() | (string() << n)
        pool.append(root)
        for _ in range(5):
            sh = n * int(rng.randint(2))
            occ = [p for p in range(n) if (root >> (p + sh)) & 1]
            emp = [q for q in range(n) if not (root >> (q + sh)) & 1]
            pool.append(root ^ (1 << (occ[rng.randint(len(occ))] + sh)) ^ (1 << (emp[rng.randint(len(emp))] + sh)))
    pool = np.array(sorted(set(pool)), dtype=np.uint64)
    assert 590 <= pool.size <= 600
    da, db = pool[rng.rand(pool.size) < 0.75], pool[rng.rand(pool.size) < 0.75]
    da, db = da[rng.permutation(da.size)], db[rng.permutation(db.size)]
    va, vb = rng.standard_normal(da.size), rng.standard_normal(db.size)
    va[::37] = 0.0
    vb[::41] = 0.0
    assert 0.4 * pool.size < np.intersect1d(da, db).size < 0.7 * pool.size
    ea, eb = Engine(mol), Engine(mol)
    for e in (ea, eb):
        e.setup(**dict(SMALL, max_dets=4000))
    ea.vec_load(da, va)
    eb.vec_load(db, vb)
    a, b = _as_map(da, va), _as_map(db, vb)
    r_ab = ea.rdm1(eb)
    ref = _reference(a, b, n)
    _check("(a,b)", r_ab, ref)
    _check("(b,a)", eb.rdm1(ea), _reference(b, a, n))
    irr = np.asarray(mol.irreps)
    forbidden = irr[:, None] != irr[None, :]
    print(f"{int((r_ab.gamma[forbidden] != 0).sum())} non-zero bins between orbitals of different irreps, {r_ab.n_hits} hits of {r_ab.n_terms}")
    assert np.any(r_ab.gamma[forbidden] != 0) and np.any(ref["gamma"][forbidden] != 0)
    for e in (ea, eb):
        e.close()


# ------------------------------------------------------------------ 4. many chunks and more than one level of the fold
def test_many_chunks_and_two_levels(Engine, mols):
    """N2 shape, seeds 1 and 2, 20 iterations at vec_nonz = mat_nonz = 20000: some 34 000 positions of which 20 000 are non-zero -- more
    than RD_FAN workgroups of RD_BPOS positions, so the fold has two levels, and a last workgroup that is not full."""
    mol = mols("N2")
    par = dict(epsilon=0.01, vec_nonz=20000, mat_nonz=20000, max_dets=160000, target_norm=10000.0, initiator=0.0, distribution="HB_unnorm")
    ea, eb = Engine(mol), Engine(mol)
    ea.setup(seed=1, **par)
    eb.setup(seed=2, **par)
    ea.iterate(20)
    eb.iterate(20)
    for e in (ea, eb):
        size = e.vec_info()[0]
        assert RD_BPOS * RD_FAN < size <= RD_BPOS * RD_FAN * RD_FAN and size % RD_BPOS != 0 and size % (RD_BPOS * RD_FAN) > RD_BPOS, size
    (da, va), (db, vb) = ea.vector(), eb.vector()
    a, b = _as_map(da, va), _as_map(db, vb)
    assert da.size - len(a) > 1000          # holes and zeros among the positions
    r_ab, r_ba = ea.rdm1(eb), eb.rdm1(ea)
    ref = _reference(a, b, mol.n_orb)
    _check("(a,b)", r_ab, ref)
    _check_gamma("(b,a) transposed", r_ba.gamma.T, ref)      # the same terms, enumerated from the other side
    _check_trace("(a,b)", r_ab, ref, mol.n_elec)
    assert r_ab.n_terms == len(a) * 210 and r_ba.n_terms == len(b) * 210 and r_ab.n_hits == r_ba.n_hits
    assert _same_bits(ea.rdm1(eb), r_ab) and _same_bits(eb.rdm1(ea), r_ba)
    for e in (ea, eb):
        e.close()


# ------------------------------------------------------------------ 5. tie to fries_h_dot
def test_tie_to_h_dot(Engine, mols):
    """With all two-electron integrals zero H is the one-body operator h_core: h_dot(a, b).h + hf_energy * ovlp = sum(h_core * gamma(a, b)).
    The allowance is the two calls' rounding bounds added: (n_hits + n_src + 8) u abs_sum of the h_dot result plus sum_pq |h_pq| * bound_pq,
    and 4 u times the magnitudes this test's own arithmetic adds up (the products h_pq * gamma_pq, hf_energy * ovlp and the final sum).  Vectors from vec_load (the pool
    of the Ne runs' determinants), so that the heat-bath tables are never used."""
    mol = mols("Ne")
    one_body = dataclasses.replace(mol, eris=np.zeros_like(mol.eris))
    src_a, src_b = pc.ne_pair(Engine, mol)
    (da, va), (db, vb) = src_a.vector(), src_b.vector()
    src_a.close()
    src_b.close()
    ea, eb = Engine(one_body), Engine(one_body)
    for e in (ea, eb):
        e.setup(**dict(SMALL, max_dets=4000))
    ea.vec_load(da[va != 0], va[va != 0])
    eb.vec_load(db[vb != 0], vb[vb != 0])
    hd, rd = ea.h_dot(eb), ea.rdm1(eb)
    ref = _reference(_as_map(da, va), _as_map(db, vb), mol.n_orb)
    _check("(a,b)", rd, ref)
    h_core = np.asarray(mol.h_core)
    prods = (h_core * rd.gamma).ravel()
    got = math.fsum(prods)
    want = hd.h + ea.hf_energy * hd.ovlp
    allow = (hd.n_hits + hd.n_src + 8) * U * hd.abs_sum + float(np.sum(np.abs(h_core) * ref["bound"])) + 4 * U * (float(np.sum(np.abs(prods))) + abs(ea.hf_energy * hd.ovlp) + abs(hd.h))
    print(f"sum(h_core * gamma) {got!r}; h + hf_en * ovlp {want!r}; difference {abs(got - want):.3e}; allowance {allow:.3e}; h_dot hits {hd.n_hits}, rdm1 hits {rd.n_hits}")
    assert hd.n_hits > 0 and rd.n_hits >= hd.n_hits
    assert abs(got - want) <= allow
    for e in (ea, eb):
        e.close()


# ------------------------------------------------------------------ 6. the real reference
def _read_fixture(name):
    """tests/golden/rdm1_ref_<name>.txt (written by tests/scripts/gen_rdm1_golden.cpp): the two vectors, <a|b> and the reference's
    internal_dot(1, 2) after one_elec_op(des, cre) for a dozen pairs"""
    a, b, refs, ovlp, n_orb, n_elec = {}, {}, [], None, 0, 0
    with open(os.path.join(ROOT, "tests", "golden", f"rdm1_ref_{name}.txt")) as f:
        for line in f:
            t = line.split()
            if not t or t[0].startswith("#"):
                continue
            if t[0] == "NORB":
                n_orb, n_elec = int(t[1]), int(t[3])
            elif t[0] in ("A", "B"):
                (a if t[0] == "A" else b)[int(t[1])] = float.fromhex(t[2])
            elif t[0] == "OVLP":
                ovlp = float.fromhex(t[1])
            elif t[0] == "REF":
                refs.append((int(t[1]), int(t[2]), float.fromhex(t[3])))
    return n_orb, n_elec, a, b, ovlp, refs


def test_against_the_reference_one_elec_op(Engine, mols):
    """The reference accumulates in arrival order, so the bits need not agree: the bound of the module docstring applies."""
    mol = mols("Ne")
    n_orb, n_elec, a, b, ovlp, refs = _read_fixture("ne")
    assert (n_orb, n_elec) == (mol.n_orb, mol.n_elec) and len(refs) >= 12
    ea, eb = Engine(mol), Engine(mol)
    for e in (ea, eb):
        e.setup(**dict(SMALL, max_dets=4000))
    ea.vec_load(np.array(list(a), dtype=np.uint64), np.array(list(a.values())))
    eb.vec_load(np.array(list(b), dtype=np.uint64), np.array(list(b.values())))
    res = ea.rdm1(eb)
    ref = _reference(a, b, n_orb)
    _check("(a,b)", res, ref)
    assert abs(res.ovlp - ovlp) <= 2 * ref["bound_ov"]
    irr = np.asarray(mol.irreps)
    n_nonzero = n_cross = 0
    for des, cre, want in refs:
        got, bound = res.gamma[cre, des], 2 * ref["bound"][cre, des]        # (the reference's own sum has the same bound against the exact one)
        print(f"des {des} cre {cre} (irreps {irr[des]}, {irr[cre]}): device {got!r} reference {want!r} err {abs(got - want):.3e} bound {bound:.3e}")
        assert des != cre and abs(got - want) <= bound, (des, cre)
        n_nonzero += want != 0
        n_cross += irr[des] != irr[cre]
    assert n_nonzero >= 4 and n_cross >= 3
    for e in (ea, eb):
        e.close()


# ------------------------------------------------------------------ 7. refusals
def _rdm1(a, b):
    return a.rdm1(b)


def test_refusals_launch_nothing(Engine, mols):
    from fries_amd.engine import Rdm1Result
    mol = mols("Ne")
    plain = Engine(mol)
    plain.setup(**SMALL)
    pc.check_common_refusals(Engine, mols, plain, _rdm1, "fries_rdm1", Rdm1Result, np.zeros((mol.n_orb, mol.n_orb)))
    pc.check_density_matrix_refusals(Engine, plain, _rdm1, "fries_rdm1")
    plain.close()


# ------------------------------------------------------------------ 8. the estimator reads, and only reads
def test_estimator_does_not_disturb_the_run(Engine, mols):
    pc.check_run_undisturbed(Engine, mols("Ne"), _rdm1)


# ------------------------------------------------------------------ 9. device memory
def test_rdm1_returns_its_device_memory(Engine, mols):
    pc.check_device_memory_returned(Engine, mols("Ne"), _rdm1, "fries_rdm1")


# ------------------------------------------------------------------ 10. FriReplicas
def test_replicas_pair_rdm1(Engine, mols):
    from fries_amd.replicas import FriReplicas
    mol = mols("Ne")
    par = _ne_run()
    seed = par.pop("seed")
    reps = FriReplicas(mol, 3, seed, **par)
    reps.iterate(20)
    got = reps.pair_rdm1()
    assert len(got) == 3 and reps.pairs() == [(0, 1), (0, 2), (1, 2)]
    nz = [e.vec_info()[1] for e in reps.engines]
    for (r, s), g in zip(reps.pairs(), got):
        if nz[r] <= nz[s]:
            want = reps.engines[r].rdm1(reps.engines[s])
            assert _same_bits(g, want), (r, s)
        else:
            want = reps.engines[s].rdm1(reps.engines[r])
            assert np.array_equal(g.gamma, want.gamma.T) and g[1:] == want[1:], (r, s)
        assert g.gamma.shape == (mol.n_orb, mol.n_orb) and g.n_hits > 0 and g.ovlp != 0
        # the trace: n_elec, within the rounding bound of the diagonal bins (a_i b_i per occupied spin orbital: n_elec terms per common determinant)
        d, v = reps.engines[r].vector()
        d2, v2 = reps.engines[s].vector()
        ref = _reference(_as_map(d, v), _as_map(d2, v2), mol.n_orb)
        _check_gamma(f"pair ({r},{s})", g.gamma, ref)
        n_e = g.expectation(np.eye(mol.n_orb))
        bound = (float(np.trace(ref["bound"])) + mol.n_elec * ref["bound_ov"]) / abs(ref["ovlp"]) + 4 * mol.n_elec * U * mol.n_elec
        print(f"pair ({r},{s}): expectation(identity) {n_e!r} bound {bound:.3e}")
        assert abs(n_e - mol.n_elec) <= bound
    for e in reps.engines:
        self_pair = e.rdm1()
        occ = self_pair.natural_occupations()
        print(f"natural occupations: largest {occ[0]!r} smallest {occ[-1]!r} sum {occ.sum()!r}")
        assert occ.shape == (mol.n_orb,) and np.all(np.diff(occ) <= 0)
        assert abs(occ.sum() - mol.n_elec) <= 1e-12 and occ.min() >= -1e-12 and occ.max() <= 2 + 1e-12
    reps.close()


# ------------------------------------------------------------------ 11. the command line
def test_command_line_repl_rdm1(Engine, mols, tmp_path):
    from fries_amd import build
    mol = mols("Ne")
    par = _ne_run()
    seed = 20250215
    fc = str(tmp_path / "mol.FCIDUMP")
    fcidump.write_fcidump(fc, mol)
    dirs = {k: str(tmp_path / k) + "/" for k in ("with", "without", "one")}
    for d in dirs.values():
        os.makedirs(d)
    repl = ["--replicas", "2", "--repl_every", "10"]
    pc.run(pc.cmd(build.DRIVER, fc, mol, par, 20, dirs["with"], seed) + repl + ["--repl_rdm1", "1"])
    pc.run(pc.cmd(build.DRIVER, fc, mol, par, 20, dirs["without"], seed) + repl)
    with_, without = pc.tree(dirs["with"]), pc.tree(dirs["without"])
    assert sorted(set(with_) - set(without)) == ["replrdm1.txt"] and not set(without) - set(with_)
    assert {"repliter.txt", "replnum.txt", "replden.txt", os.path.join("replica0", "dets0.dat"), os.path.join("replica1", "projnum.txt")} <= set(without)
    for name, blob in without.items():
        assert with_[name] == blob, name
    lines = with_["replrdm1.txt"].decode().split("\n")
    assert lines[-1] == "" and len(lines) == 3
    rows = [np.array([float(x) for x in ln.split(",")]) for ln in lines[:2]]
    assert all(r.size == mol.n_orb ** 2 for r in rows)
    # the last line against fries_rdm1 on the two final checkpoints (positions differ after a load, so the bits may)
    engs, maps = [], []
    for r in range(2):
        e = Engine(mol)
        e.setup(**dict(par, seed=seed + r))
        d, v = pc.saved_vector(dirs["with"] + f"replica{r}/", mol)
        e.vec_load(d, v)
        engs.append(e)
        maps.append(_as_map(d, v))
    swap = engs[0].vec_info()[1] > engs[1].vec_info()[1]
    res = engs[1].rdm1(engs[0]).transposed() if swap else engs[0].rdm1(engs[1])
    ref = _reference(maps[0], maps[1], mol.n_orb)
    _check_gamma("checkpoints", res.gamma, ref)
    printed = rows[1].reshape(mol.n_orb, mol.n_orb)
    _check_gamma("replrdm1.txt, last line", printed, ref)            # 17 digits round-trip, so the printed matrix is within the same bound of the reference
    assert np.all(np.abs(printed - res.gamma) <= 2 * ref["bound"])
    assert abs(np.trace(printed) - mol.n_elec * float(with_["replden.txt"].decode().split()[-1])) <= 2 * (float(np.trace(ref["bound"])) + mol.n_elec * ref["bound_ov"]) + 4 * mol.n_elec * U * abs(np.trace(printed))
    # one replica: the pair (0, 0)
    pc.run(pc.cmd(build.DRIVER, fc, mol, par, 20, dirs["one"], seed) + ["--replicas", "1", "--repl_every", "10", "--repl_rdm1", "1"])
    one = pc.tree(dirs["one"])["replrdm1.txt"].decode().split("\n")
    assert len(one) == 3 and one[-1] == ""
    self_printed = np.array([float(x) for x in one[1].split(",")]).reshape(mol.n_orb, mol.n_orb)
    _check_gamma("one replica", self_printed, _reference(maps[0], maps[0], mol.n_orb))
    for e in engs:
        e.close()
