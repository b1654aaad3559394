"""-m gpu: the two-body density matrix between replicas, fries_rdm2 (csrc/rdm2.hip), and what is built on it.

The reference of every numerical check is formed here from the definition, over Python integers and independent of the device's
enumerate-and-probe: a join on (N-2)-electron intermediates.  For every non-zero a_i and every ordered pair (P, R) of occupied spin
orbitals, c_R c_P |i> with its sign (every operator counts the occupied bits below it at its turn); the same for b with (Q, S); where
the intermediates coincide and spin(P) = spin(Q), spin(R) = spin(S), the product a_i b_j * signs goes to bin (p, q, r, s).  Per bin
the terms are summed with math.fsum.  With u = 2**-53 every term is one rounded product, and a sum of n doubles in ANY order is within
(n - 1) u S of the exact one (S = the sum of the magnitudes): |device - reference| <= (n + 8) u S per bin, whatever order the device adds
in; the 8 covers the products, fsum's own rounding and the one addition of the two halves of a bin (the device accumulates one of the
records (p,q,r,s) / (r,s,p,q) of every term and adds the matrix to its pair transpose).  ovlp and abs_sum are bounded the same way.
Worst cases, not measured."""
import math
import os

import numpy as np
import pytest

import pair_common as pc
import test_gpu_rdm1 as t1
from fries_amd import fcidump
from pair_common import SMALL, U, as_map as _as_map, same_bits as _same_bits

pytestmark = pytest.mark.gpu
R2_BPOS, R2_WPOS = 32, 8          # the geometry of csrc/rdm2_plan.hpp: positions per workgroup and per wave


@pytest.fixture(scope="module")
def Engine():
    from fries_amd.engine import FriEngine
    return FriEngine


def _below(d, x):
    return bin(d & ((1 << x) - 1)).count("1")


def _intermediates(vec, n_orb):
    """c_second c_first |i> for every ordered pair of occupied spin orbitals: intermediate -> [(first, second, signed value, i)]"""
    out = {}
    for i, ai in vec.items():
        occ = [P for P in range(2 * n_orb) if (i >> P) & 1]
        for P in occ:
            s1 = _below(i, P)
            i1 = i ^ (1 << P)
            for R in occ:
                if R != P:
                    out.setdefault(i1 ^ (1 << R), []).append((P, R, -ai if (s1 + _below(i1, R)) & 1 else ai, i))
    return out


def _spin_conserving(i, j, n_orb):
    """0: not connected; 1 / 2: one / two spin-conserving replacements apart"""
    low = (1 << n_orb) - 1
    x = i ^ j
    lvl = 0
    for sh in (0, n_orb):
        out_, in_ = bin((i & x) >> sh & low).count("1"), bin((j & x) >> sh & low).count("1")
        if out_ != in_:
            return 0
        lvl += out_
    return lvl if lvl in (1, 2) else 0


def _comb2(k):
    return k * (k - 1) // 2


def _reference(a, b, n_orb):
    n = n_orb
    terms, classes = {}, {}
    ia, ib = _intermediates(a, n), _intermediates(b, n)
    for k, la in ia.items():
        lb = ib.get(k)
        if lb is None:
            continue
        for P, R, x, i in la:
            for Q, S, y, j in lb:
                if P // n != Q // n or R // n != S // n:
                    continue
                key = (P % n, Q % n, R % n, S % n)
                terms.setdefault(key, []).append(x * y)
                if i == j:
                    cls = "diagonal"
                elif bin(i ^ j).count("1") == 2:
                    cls = "single exchange" if (Q == R or P == S) else "single direct"
                else:
                    cls = "double same" if P // n == R // n else "double opposite"
                classes.setdefault(cls, set()).add(key)
    gamma2, mag, cnt = np.zeros((n,) * 4), np.zeros((n,) * 4), np.zeros((n,) * 4, dtype=np.int64)
    for key, ts in terms.items():
        gamma2[key], mag[key], cnt[key] = math.fsum(ts), math.fsum(abs(t) for t in ts), len(ts)
    # counts, the overlap and abs_sum: straight from the vectors
    low = (1 << n) - 1
    n_terms, hits, ov_terms, rec = 0, [], [], {}
    for i, ai in a.items():
        ha, hb = bin(i & low).count("1"), bin(i >> n).count("1")
        n_terms += ha * (n - ha) + hb * (n - hb) + _comb2(ha) * _comb2(n - ha) + _comb2(hb) * _comb2(n - hb) + ha * (n - ha) * hb * (n - hb)
        r = 0
        for j, bj in b.items():
            if i == j:
                ov_terms.append(ai * bj)
                r += _comb2(ha + hb) + _comb2(ha) + _comb2(hb)
                continue
            lvl = _spin_conserving(i, j, n)
            if lvl:
                hits.append(abs(ai * bj))
                if lvl == 1:
                    beta = ((i & ~j) >> n) != 0
                    r += (ha + hb - 1) + ((hb if beta else ha) - 1)
                else:
                    r += 2 if (((i & ~j) & low) == 0 or ((i & ~j) >> n) == 0) else 1
        rec[i] = r          # the bin records the device expands source i to (csrc/rdm2.hip): what the chunks are cut by
    return dict(gamma2=gamma2, bound=(cnt + 8) * U * mag, cnt=cnt, classes=classes, ovlp=math.fsum(ov_terms),
                bound_ov=(len(ov_terms) + 8) * U * math.fsum(abs(t) for t in ov_terms), abs_sum=math.fsum(hits), bound_abs=(len(hits) + 8) * U * math.fsum(hits),
                n_src=len(a), n_terms=n_terms, n_hits=len(hits), rec=rec)


def _check_gamma(tag, g, ref, transposed=False):
    want, bound = (ref["gamma2"].transpose(1, 0, 3, 2), ref["bound"].transpose(1, 0, 3, 2)) if transposed else (ref["gamma2"], ref["bound"])
    err = np.abs(g - want)
    worst = np.unravel_index(np.argmax(np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), err)), err.shape)
    print(f"{tag}: {int((want != 0).sum())} non-zero bins, {int(ref['cnt'].sum())} terms; bin closest to its bound {worst}: device {g[worst]!r} reference {want[worst]!r} err {err[worst]:.3e} bound {bound[worst]:.3e}")
    assert g.shape == want.shape
    assert np.all(err <= bound), tag


def _check(tag, res, ref):
    print(f"{tag}: n_src {res.n_src} n_terms {res.n_terms} n_hits {res.n_hits}; ovlp {res.ovlp!r} err {abs(res.ovlp - ref['ovlp']):.3e} bound {ref['bound_ov']:.3e}; "
          f"abs_sum {res.abs_sum!r} err {abs(res.abs_sum - ref['abs_sum']):.3e} bound {ref['bound_abs']:.3e}")
    assert (res.n_src, res.n_terms, res.n_hits) == (ref["n_src"], ref["n_terms"], ref["n_hits"]), (tag, ref["n_src"], ref["n_terms"], ref["n_hits"])
    _check_gamma(tag, res.gamma2, ref)
    assert abs(res.ovlp - ref["ovlp"]) <= ref["bound_ov"], tag
    assert abs(res.abs_sum - ref["abs_sum"]) <= ref["bound_abs"], tag
    # pair symmetry, bit for bit
    assert np.array_equal(res.gamma2, res.gamma2.transpose(2, 3, 0, 1)), tag


def _check_full_trace(tag, res, ref, n_elec):
    """sum_pr Gamma[p,p,r,r] = n_elec (n_elec - 1) <a|b>: the bins' bounds, the overlap's bound times the factor, and 2 u per addition of this
    test's own sum of n_orb^2 bins"""
    n = res.gamma2.shape[0]
    diag = np.einsum("pprr->pr", res.gamma2)
    tr, f = math.fsum(diag.ravel()), n_elec * (n_elec - 1)
    bound = float(np.einsum("pprr->", ref["bound"])) + f * ref["bound_ov"] + 4 * U * (float(np.abs(diag).sum()) + abs(f * ref["ovlp"]))
    print(f"{tag}: full trace {tr!r} n_elec (n_elec - 1) ovlp {f * res.ovlp!r} bound {bound:.3e} ({n * n} bins)")
    assert abs(tr - f * res.ovlp) <= bound, tag


def _all_checks(ea, eb, a, b, n_orb, n_elec):
    r_ab, r_ba, r_aa = ea.rdm2(eb), eb.rdm2(ea), ea.rdm2()
    ref_ab, ref_aa = _reference(a, b, n_orb), _reference(a, a, n_orb)
    _check("(a,b)", r_ab, ref_ab)
    _check("(b,a)", r_ba, _reference(b, a, n_orb))
    _check("(a,a)", r_aa, ref_aa)
    # Gamma(a, b)[p,q,r,s] = Gamma(b, a)[q,p,s,r]: the same products enumerated from the other side, within the bound of the same reference
    _check_gamma("(b,a) transposed", r_ba.transposed().gamma2, ref_ab)
    _check_full_trace("(a,b)", r_ab, ref_ab, n_elec)
    _check_full_trace("(a,a)", r_aa, ref_aa, n_elec)
    for _ in range(3):
        assert _same_bits(ea.rdm2(eb), r_ab) and _same_bits(eb.rdm2(ea), r_ba) and _same_bits(ea.rdm2(ea), r_aa)
    return r_ab, ref_ab


# ------------------------------------------------------------------ 1. whole space
def test_whole_space_min4(Engine, mols):
    """2 electrons in 4 orbitals, C1: all 16 determinants in both vectors, in different orders, two exact zeros each"""
    mol = mols("MIN4")
    ea, eb, _, (da, va), (db, vb) = pc.min4_pair(Engine, mol, 20252)
    r_ab, ref = _all_checks(ea, eb, _as_map(da, va), _as_map(db, vb), mol.n_orb, mol.n_elec)
    assert r_ab.gamma2.shape == (4, 4, 4, 4) and r_ab.n_src == 14 and r_ab.n_terms == 14 * (2 * 1 * 3 + 0 + 1 * 9)
    assert set(ref["classes"]) == {"diagonal", "single direct", "double opposite"}      # no same-spin pair in this space
    for e in (ea, eb):
        e.close()


# ------------------------------------------------------------------ 2. compressed vectors with holes
_ne_pair = pc.ne_pair


def test_sparse_vectors_with_holes(Engine, mols):
    """Two Ne runs (seeds 1 and 2), 25 iterations at vec_nonz = mat_nonz = 150: compressed vectors with released positions; most targets are
    not in the other vector.  The first test of same-spin doubles and of exchange spectators."""
    mol = mols("Ne")
    ea, eb = _ne_pair(Engine, mol)
    (da, va), (db, vb) = ea.vector(), eb.vector()
    a, b = _as_map(da, va), _as_map(db, vb)
    assert len(a) < da.size or len(b) < db.size or ea.vec_info()[2] + eb.vec_info()[2] > 0, "no released position in either vector"
    r_ab, ref = _all_checks(ea, eb, a, b, mol.n_orb, mol.n_elec)
    assert 0 < r_ab.n_hits < r_ab.n_terms
    assert (mol.n_elec, mol.n_orb) == (8, 22)
    assert r_ab.n_terms == r_ab.n_src * (2 * 4 * 18 + 2 * math.comb(4, 2) * math.comb(18, 2) + 16 * 18 ** 2)
    print(f"{da.size} and {db.size} positions, {len(a)} and {len(b)} non-zero; classes {sorted((k, len(v)) for k, v in ref['classes'].items())}")
    assert {"double same", "single exchange", "double opposite", "single direct", "diagonal"} <= set(ref["classes"])
    for e in (ea, eb):
        e.close()


# ------------------------------------------------------------------ 3. vectors that ignore symmetry
def test_vectors_that_ignore_symmetry(Engine, mols):
    """Ne shape, loaded with vec_load: 30 random roots (n_elec / 2 electrons per spin, RandomState(11)) plus three random single, three
    same-spin double and three opposite-spin double replacements of each, with no regard to the irreps: about 300 determinants.  a and b
    take 75 % of the pool each; values are normal with a few exact zeros.  fries_rdm2 consults no symmetry table."""
    mol = mols("Ne")
    n, half = mol.n_orb, mol.n_elec // 2
    rng = np.random.RandomState(11)

    def string():
        return sum(1 << int(p) for p in rng.choice(n, half, replace=False))

    def replace(det, sh, k):
        occ = [p for p in range(n) if (det >> (p + sh)) & 1]
        emp = [q for q in range(n) if not (det >> (q + sh)) & 1]
        for p in rng.choice(occ, k, replace=False):
            det ^= 1 << (int(p) + sh)
        for q in rng.choice(emp, k, replace=False):
            det ^= 1 << (int(q) + sh)
        return det

    pool = []
    for _ in range(30):
        root = string() | (string() << n)
        pool.append(root)
        for _ in range(3):
            pool.append(replace(root, n * int(rng.randint(2)), 1))
            pool.append(replace(root, n * int(rng.randint(2)), 2))
            pool.append(replace(replace(root, 0, 1), n, 1))
    pool = np.array(sorted(set(pool)), dtype=np.uint64)
    assert 280 <= pool.size <= 300
    da, db = pool[rng.rand(pool.size) < 0.75], pool[rng.rand(pool.size) < 0.75]
    da, db = da[rng.permutation(da.size)], db[rng.permutation(db.size)]
    va, vb = rng.standard_normal(da.size), rng.standard_normal(db.size)
    va[::37] = 0.0
    vb[::41] = 0.0
    ea, eb = Engine(mol), Engine(mol)
    for e in (ea, eb):
        e.setup(**dict(SMALL, max_dets=4000))
    ea.vec_load(da, va)
    eb.vec_load(db, vb)
    a, b = _as_map(da, va), _as_map(db, vb)
    ref = _reference(a, b, n)
    _check("(a,b)", ea.rdm2(eb), ref)
    _check("(b,a)", eb.rdm2(ea), _reference(b, a, n))
    g = ref["gamma2"]
    for cls in ("double same", "double opposite", "single exchange", "diagonal"):
        bins = ref["classes"].get(cls, set())
        assert any(g[k] != 0 for k in bins), cls
    assert any(g[k] != 0 and k[1] == k[2] and k[0] != k[3] for k in ref["classes"]["single exchange"])      # an exchange bin [p,k,k,q]
    irr = np.asarray(mol.irreps).astype(np.int64)
    prod = irr[:, None, None, None] ^ irr[None, :, None, None] ^ irr[None, None, :, None] ^ irr[None, None, None, :]
    print(f"{int(((g != 0) & (prod != 0)).sum())} non-zero bins whose irreps do not multiply to the identity, of {int((g != 0).sum())}")
    assert np.any((g != 0) & (prod != 0))
    for e in (ea, eb):
        e.close()


# ------------------------------------------------------------------ 4. several chunks
def _cut(wg_rec, cap):
    """the greedy cut of csrc/rdm2_plan.hpp: records per chunk"""
    chunks, cur = [], 0
    for k, t in enumerate(wg_rec):
        assert t <= cap
        if cur + t > cap:
            chunks.append(cur)
            cur = 0
        cur += t
    return chunks + [cur]


def test_several_chunks(Engine, mols, monkeypatch):
    """The engines of test 2 under a FRIES_RDM2_RECORDS so small that the call needs at least three chunks with a partial last one: the
    largest need of one workgroup (R2_BPOS positions), from the records the reference counts per source."""
    mol = mols("Ne")
    ea, eb = _ne_pair(Engine, mol)
    (da, va), (db, vb) = ea.vector(), eb.vector()
    a, b = _as_map(da, va), _as_map(db, vb)
    ref = _reference(a, b, mol.n_orb)
    whole = ea.rdm2(eb)
    _check("one chunk", whole, ref)
    wg_rec = [sum(ref["rec"].get(int(d), 0) for d, v in zip(da[k:k + R2_BPOS], va[k:k + R2_BPOS]) if v != 0) for k in range(0, da.size, R2_BPOS)]
    cap = max(wg_rec)
    chunks = _cut(wg_rec, cap)
    print(f"{da.size} positions, records per workgroup {wg_rec}; capacity {cap}: chunks of {chunks} records")
    assert len(chunks) >= 3 and 0 < chunks[-1] < cap
    monkeypatch.setenv("FRIES_RDM2_RECORDS", str(cap))
    ca, cb = _ne_pair(Engine, mol)
    monkeypatch.setenv("FRIES_RDM2_RECORDS", str(cap - 1))
    tight = Engine(mol)
    monkeypatch.delenv("FRIES_RDM2_RECORDS")
    tight.setup(seed=1, **pc.NE_PAIR)
    tight.iterate(25)
    for e in (ca, tight):
        d, v = e.vector()
        assert d.tobytes() == da.tobytes() and v.tobytes() == va.tobytes()
    n0 = ca.kernel_launches
    chunked = ca.rdm2(cb)
    # the counting pass, then per chunk the emitting pass, three launches per 8-bit pass of the sort (22^4 bins: 3 passes) and the two of the sum
    assert ca.kernel_launches - n0 == 1 + len(chunks) * (1 + 3 * 3 + 2)
    _check("chunked", chunked, ref)
    assert np.all(np.abs(chunked.gamma2 - whole.gamma2) <= 2 * ref["bound"])
    assert chunked[1:] == whole[1:]
    for _ in range(3):
        assert _same_bits(ca.rdm2(cb), chunked)
    # a capacity below one workgroup's need: refused with a message after the counting pass -- the one launch that tells the need --,
    # before anything is allocated for or written to the records
    n0, n1 = tight.kernel_launches, cb.kernel_launches
    with pytest.raises(RuntimeError, match="FRIES_RDM2_RECORDS") as ex:
        tight.rdm2(cb)
    print(ex.value)
    assert "fries_rdm2" in str(ex.value) and str(cap) in str(ex.value) and str(cap - 1) in str(ex.value)
    assert (tight.kernel_launches - n0, cb.kernel_launches - n1) == (1, 0)
    for e in (ea, eb, ca, cb, tight):
        e.close()


# ------------------------------------------------------------------ 5. ties to what exists
def _eri4(mol):
    n = mol.n_orb
    eris = np.asarray(mol.eris)
    out = np.zeros((n,) * 4)
    for p, q, r, s in np.ndindex(n, n, n, n):
        out[p, q, r, s] = eris[fcidump.eri_index(p, q, r, s)]
    return out


def test_ties_to_rdm1_and_h_dot(Engine, mols):
    """Ne vectors from runs, full integrals.  sum_r Gamma[p,q,r,r] = (n_elec - 1) gamma[p,q] with fries_rdm1's gamma, and
    sum(h_core gamma) + 1/2 sum(eri4 Gamma) = fries_h_dot's h + hf_energy * ovlp.  The allowances are the calls' rounding bounds added:
    the bins' bounds of both references weighted as the identity weights them, (n_hits + n_src + 8) u abs_sum of the h_dot result, and
    4 u times the magnitudes this test's own arithmetic adds up."""
    mol = mols("Ne")
    ea, eb = _ne_pair(Engine, mol)
    (da, va), (db, vb) = ea.vector(), eb.vector()
    a, b = _as_map(da, va), _as_map(db, vb)
    n, n_elec = mol.n_orb, mol.n_elec
    r2, r1, hd = ea.rdm2(eb), ea.rdm1(eb), ea.h_dot(eb)
    ref2, ref1 = _reference(a, b, n), t1._reference(a, b, n)
    _check("(a,b)", r2, ref2)
    assert r2.ovlp == r1.ovlp or abs(r2.ovlp - r1.ovlp) <= 2 * ref2["bound_ov"]
    # the partial trace
    pt = np.einsum("pqrr->pq", r2.gamma2)
    allow = np.einsum("pqrr->pq", ref2["bound"]) + (n_elec - 1) * ref1["bound"] + 4 * U * (np.einsum("pqrr->pq", np.abs(r2.gamma2)) + (n_elec - 1) * np.abs(r1.gamma))
    err = np.abs(pt - (n_elec - 1) * r1.gamma)
    worst = np.unravel_index(np.argmax(err - allow), err.shape)
    print(f"partial trace: worst bin {worst}: {pt[worst]!r} against {(n_elec - 1) * r1.gamma[worst]!r}, err {err[worst]:.3e} allowance {allow[worst]:.3e}; {int((pt != 0).sum())} non-zero")
    assert np.all(err <= allow) and np.any(pt != 0)
    assert np.all(np.abs(r2.partial_trace(n_elec) - r1.gamma) <= allow / (n_elec - 1) + 2 * U * np.abs(r1.gamma))
    # the energy
    h_core, eri4 = np.asarray(mol.h_core), _eri4(mol)
    p1, p2 = (h_core * r1.gamma).ravel(), (0.5 * eri4 * r2.gamma2).ravel()
    got = math.fsum(p1) + math.fsum(p2)
    want = hd.h + ea.hf_energy * hd.ovlp
    allow = ((hd.n_hits + hd.n_src + 8) * U * hd.abs_sum + float(np.sum(np.abs(h_core) * ref1["bound"])) + 0.5 * float(np.sum(np.abs(eri4) * ref2["bound"]))
             + 4 * U * (float(np.sum(np.abs(p1))) + float(np.sum(np.abs(p2))) + abs(ea.hf_energy * hd.ovlp) + abs(hd.h)))
    print(f"sum(h gamma) + 1/2 sum(eri Gamma) {got!r}; h + hf_en * ovlp {want!r}; difference {abs(got - want):.3e}; allowance {allow:.3e}; h_dot hits {hd.n_hits}, rdm2 hits {r2.n_hits}")
    assert hd.n_hits > 0 and r2.n_hits >= hd.n_hits
    assert abs(got - want) <= allow
    assert abs(r2.energy(h_core, eri4, r1.gamma) - want / hd.ovlp) <= 2 * allow / abs(hd.ovlp) + 4 * U * abs(want / hd.ovlp)
    for e in (ea, eb):
        e.close()


def test_spin_squared_of_the_open_shell_pair(Engine, mols):
    """|0 alpha 1 beta> +- |1 alpha 0 beta> on MIN4: plus is the singlet (0), minus the triplet component (2).  Small integers: exact."""
    mol = mols("MIN4")
    n = mol.n_orb
    dets = np.array([(1 << 0) | (1 << (n + 1)), (1 << 1) | (1 << (n + 0))], dtype=np.uint64)
    e = Engine(mol)
    e.setup(epsilon=0.01, vec_nonz=50, mat_nonz=50, max_dets=1000, seed=3, distribution="HB_unnorm")
    for sign, want in ((1.0, 0.0), (-1.0, 2.0)):
        e.vec_load(dets, np.array([1.0, sign]))
        r = e.rdm2()
        print(f"sign {sign}: ovlp {r.ovlp} <S^2> {r.spin_squared(mol.n_elec)}")
        assert r.ovlp == 2.0 and r.spin_squared(mol.n_elec) == want
    e.close()


# ------------------------------------------------------------------ 6. refusals
def _rdm2(a, b):
    return a.rdm2(b)


def test_refusals_launch_nothing(Engine, mols):
    from fries_amd.engine import Rdm2Result
    mol = mols("Ne")
    plain = Engine(mol)
    plain.setup(**SMALL)
    pc.check_common_refusals(Engine, mols, plain, _rdm2, "fries_rdm2", Rdm2Result, np.zeros((mol.n_orb,) * 4))
    pc.check_density_matrix_refusals(Engine, plain, _rdm2, "fries_rdm2")
    plain.close()


# ------------------------------------------------------------------ 7. the estimator reads, and only reads
def test_estimator_does_not_disturb_the_run(Engine, mols):
    pc.check_run_undisturbed(Engine, mols("Ne"), _rdm2)


# ------------------------------------------------------------------ 8. device memory
def test_rdm2_returns_its_device_memory(Engine, mols):
    pc.check_device_memory_returned(Engine, mols("Ne"), _rdm2, "fries_rdm2")


# ------------------------------------------------------------------ 9. FriReplicas
def test_replicas_pair_rdm2(Engine, mols):
    from fries_amd.replicas import FriReplicas
    mol = mols("Ne")
    par = pc.ne_run()
    seed = par.pop("seed")
    reps = FriReplicas(mol, 3, seed, **par)
    reps.iterate(20)
    got = reps.pair_rdm2()
    assert len(got) == 3 and reps.pairs() == [(0, 1), (0, 2), (1, 2)]
    nz = [e.vec_info()[1] for e in reps.engines]
    n, n_elec = mol.n_orb, mol.n_elec
    unit = np.einsum("pq,rs->pqrs", np.eye(n), np.eye(n))
    for (r, s), g in zip(reps.pairs(), got):
        if nz[r] <= nz[s]:
            assert _same_bits(g, reps.engines[r].rdm2(reps.engines[s])), (r, s)
        else:
            want = reps.engines[s].rdm2(reps.engines[r])
            assert np.array_equal(g.gamma2, want.gamma2.transpose(1, 0, 3, 2)) and g[1:] == want[1:], (r, s)
        assert g.gamma2.shape == (n,) * 4 and g.n_hits > 0 and g.ovlp != 0
        d, v = reps.engines[r].vector()
        d2, v2 = reps.engines[s].vector()
        ref = _reference(_as_map(d, v), _as_map(d2, v2), n)
        _check_gamma(f"pair ({r},{s})", g.gamma2, ref)
        # the unit operator: 1/2 sum_pr Gamma[p,p,r,r] / ovlp = n_elec (n_elec - 1) / 2, within the bins' and the overlap's bounds over |ovlp|
        # and 4 u per unit of this test's own sum and division
        pairs = n_elec * (n_elec - 1) / 2
        val = g.expectation(unit)
        bound = (0.5 * float(np.einsum("pprr->", ref["bound"])) + pairs * ref["bound_ov"]) / abs(ref["ovlp"]) + 4 * U * (0.5 * float(np.einsum("pprr->", np.abs(g.gamma2))) / abs(g.ovlp) + pairs)
        print(f"pair ({r},{s}): expectation(unit) {val!r} bound {bound:.3e}")
        assert abs(val - pairs) <= bound
    reps.close()


# ------------------------------------------------------------------ 10. the command line
def test_command_line_repl_rdm2(Engine, mols, tmp_path):
    from fries_amd import build
    mol = mols("Ne")
    par = pc.ne_run()
    seed = 20250215
    n = mol.n_orb
    fc = str(tmp_path / "mol.FCIDUMP")
    fcidump.write_fcidump(fc, mol)
    dirs = {k: str(tmp_path / k) + "/" for k in ("with", "without", "one")}
    for d in dirs.values():
        os.makedirs(d)
    repl = ["--replicas", "2", "--repl_every", "10"]
    pc.run(pc.cmd(build.DRIVER, fc, mol, par, 20, dirs["with"], seed) + repl + ["--repl_rdm2", "1"])
    pc.run(pc.cmd(build.DRIVER, fc, mol, par, 20, dirs["without"], seed) + repl)
    with_, without = pc.tree(dirs["with"]), pc.tree(dirs["without"])
    assert sorted(set(with_) - set(without)) == ["replrdm2.dat", "replrdm2e.txt"] and not set(without) - set(with_)
    for name, blob in without.items():
        assert with_[name] == blob, name
    blocks = np.frombuffer(with_["replrdm2.dat"], dtype="<f8")
    assert blocks.size == 2 * n ** 4
    last = blocks[n ** 4:].reshape((n,) * 4)
    # the last block against the reference built from the two final checkpoints
    maps = []
    for r in range(2):
        d, v = pc.saved_vector(dirs["with"] + f"replica{r}/", mol)
        maps.append(_as_map(d, v))
    ref2, ref1 = _reference(maps[0], maps[1], n), t1._reference(maps[0], maps[1], n)
    _check_gamma("replrdm2.dat, last block", last, ref2)
    assert np.array_equal(last, last.transpose(2, 3, 0, 1))
    # replrdm2e.txt: (sum(h gamma) + 1/2 sum(eri Gamma)) / ovlp against replnum / replden + hf_energy of the same meeting; the allowance as
    # in test_ties_to_rdm1_and_h_dot, over |ovlp| (the h_dot call's n_hits and abs_sum are not printed: the call is repeated on the checkpoints)
    lines = with_["replrdm2e.txt"].decode().split("\n")
    assert lines[-1] == "" and len(lines) == 3
    e_last = float(lines[1])
    num, den = (float(with_[f].decode().split()[-1]) for f in ("replnum.txt", "replden.txt"))
    engs = []
    for r in range(2):
        e = Engine(mol)
        e.setup(**dict(par, seed=seed + r))
        e.vec_load(np.array(list(maps[r]), dtype=np.uint64), np.array(list(maps[r].values())))
        engs.append(e)
    hf = engs[0].hf_energy
    hd = engs[0].h_dot(engs[1])         # the same terms as the meeting's fries_h_dot: its n_hits and abs_sum give that call's rounding bound
    for e in engs:
        e.close()
    h_core, eri4 = np.asarray(mol.h_core), _eri4(mol)
    bins = float(np.sum(np.abs(h_core) * ref1["bound"])) + 0.5 * float(np.sum(np.abs(eri4) * ref2["bound"]))
    mags = float(np.sum(np.abs(h_core * ref1["gamma"]))) + 0.5 * float(np.sum(np.abs(eri4 * ref2["gamma2"]))) + abs(hf * den) + abs(num)
    # the driver adds the n_orb^4 products one after the other: (n_orb^4 + n_orb^2) u times their magnitudes
    allow = (bins + 2 * (hd.n_hits + hd.n_src + 8) * U * hd.abs_sum + (n ** 4 + n ** 2) * U * mags) / abs(den) + 8 * U * abs(num / den + hf)
    print(f"replrdm2e.txt last value {e_last!r}; replnum / replden + hf {num / den + hf!r}; difference {abs(e_last - (num / den + hf)):.3e}; allowance {allow:.3e}")
    assert abs(e_last - (num / den + hf)) <= allow
    # one replica: the pair (0, 0)
    pc.run(pc.cmd(build.DRIVER, fc, mol, par, 20, dirs["one"], seed) + ["--replicas", "1", "--repl_every", "10", "--repl_rdm2", "1"])
    one = pc.tree(dirs["one"])
    self_blocks = np.frombuffer(one["replrdm2.dat"], dtype="<f8")
    assert self_blocks.size == 2 * n ** 4 and len(one["replrdm2e.txt"].decode().split("\n")) == 3
    _check_gamma("one replica", self_blocks[n ** 4:].reshape((n,) * 4), _reference(maps[0], maps[0], n))
