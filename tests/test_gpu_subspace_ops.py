"""-m gpu: the four operators a loop over several vectors needs beside the stepwise ones (csrc/snapshot.hip, csrc/api_vec.hip):
fries_vec_axpy_snapshot, fries_snapshot_dot, fries_vec_scale, fries_vec_one_norm, and their Python bindings.

The vectors are Ne at vec_nonz = mat_nonz = 2000 (the NE set-up of test_gpu_stepwise.py) after 5 and 8 iterations with different seeds:
cut so that they overlap only partly (the fixture `vecs` says why and how).  u = 2**-53.
  * the axpy is compared with fries_vec_add_to of the same list on a twin engine that holds the same vector in the same layout: every
    element is one add of the same two doubles in the same order, so the comparison is equality of bytes;
  * the dot against math.fsum of its products: (n_hits + 8) u abs_sum bounds ANY association order of n_hits products whose
    magnitudes sum to abs_sum (a worst case, as in test_gpu_snapshot.test_sharded_against_the_union);
  * the scale against numpy's product, as bytes; the one-norm against find_preserve's, as a double."""
import ctypes as C
import dataclasses
import math
import threading

import numpy as np
import pytest

import golden_io
from fries_amd import fcidump

pytestmark = pytest.mark.gpu
U = 2.0 ** -53
NE = dict(epsilon=0.01, vec_nonz=2000, mat_nonz=2000, max_dets=20000, target_norm=1000.0, initiator=1.0, distribution="HB_unnorm")
SMALL = dict(epsilon=0.01, vec_nonz=100, mat_nonz=100, max_dets=1000, seed=1, distribution="HB_unnorm")
SEED_A, SEED_B = 20250215, 20250216
COEFFS = (1.0, -0.37, 2.0 ** -1074)


@pytest.fixture(scope="module")
def Engine():
    from fries_amd.engine import FriEngine
    return FriEngine


@pytest.fixture(scope="module")
def Snapshot():
    from fries_amd.engine import VecSnapshot
    return VecSnapshot


def _threads(jobs):
    errs = []

    def run(j):
        try:
            j()
        except BaseException as ex:
            errs.append(ex)
    th_ = [threading.Thread(target=run, args=(j,)) for j in jobs]
    for t in th_:
        t.start()
    for t in th_:
        t.join()
    assert not errs, errs


class Sharded:
    """One frisys_mol run over P rank threads of this process (LocalGroup), as test_gpu_snapshot.Sharded"""

    def __init__(self, Engine, mol, P, seed, par, n_iter=0):
        from fries_amd.comm import LocalGroup
        par = {k: v for k, v in par.items() if k != "seed"}
        self.grp = LocalGroup(P, par["mat_nonz"])
        self.eng = [Engine(mol, device=0, comm=self.grp.comm(k, 0)) for k in range(P)]
        _threads([(lambda e=e: e.setup(seed=seed, **par)) for e in self.eng])
        if n_iter:
            _threads([(lambda e=e: e.iterate(n_iter)) for e in self.eng])

    def close(self):
        for e in self.eng:
            e.close()
        self.grp.destroy()


def _column(eng, col):
    n = eng.vec_info()[0]
    out = np.zeros(max(n, 1))
    m = C.c_size_t()
    eng._ck(eng.lib.fries_vec_column_download(eng.h, col, out.ctypes.data_as(C.c_void_p), out.size, C.byref(m)))
    return out[:m.value]


def _live(eng):
    d, v = eng.vector()
    return d[v != 0].copy(), v[v != 0].copy()


@pytest.fixture(scope="module")
def vecs(Engine, mols):
    """(dets, vals) of the two Ne vectors' live entries, in position order; computed once"""
    mol = mols("Ne")
    a, b = Engine(mol), Engine(mol)
    a.setup(seed=SEED_A, **NE)
    b.setup(seed=SEED_B, **NE)
    a.iterate(5)
    b.iterate(8)
    (da, va), (db, vb) = _live(a), _live(b)
    a.close()
    b.close()
    # At these iteration counts the budget of 2000 has not bitten yet: both runs hold the same determinants (with other values).  So
    # that the two overlap only partly, `a` keeps its first two thirds and `b` its last two thirds, each in its own position order.
    print(f"a: {da.size} entries, b: {db.size} entries, {np.intersect1d(da, db).size} in common before the cut")
    da, va = da[:2 * da.size // 3], va[:2 * va.size // 3]
    db, vb = db[db.size // 3:], vb[vb.size // 3:]
    common = np.intersect1d(da, db).size
    print(f"after the cut: a {da.size}, b {db.size}, {common} in common")
    assert 0 < common < min(da.size, db.size) and not np.array_equal(va[:8], vb[:8])
    return (da, va), (db, vb)


def _loaded(Engine, mol, dets, vals, par=NE, seed=SEED_A):
    e = Engine(mol)
    e.setup(seed=seed, **par)
    e.vec_load(dets, vals)
    return e


def _same_vectors(x, y):
    assert x.vec_info() == y.vec_info()
    (dx, vx), (dy, vy) = x.vector(), y.vector()
    assert dx.tobytes() == dy.tobytes(), "determinants differ position by position"
    assert vx.tobytes() == vy.tobytes(), "column 0 differs"
    assert _column(x, 1).tobytes() == _column(y, 1).tobytes(), "column 1 differs"


def _b_list(kind, vecs):
    (da, va), (db, vb) = vecs
    in_a = np.isin(db, da)
    if kind == "subset":
        return db[in_a], vb[in_a]
    if kind == "disjoint":
        return db[~in_a], vb[~in_a]
    if kind == "empty":
        return db[:0], vb[:0]
    return db, vb


# ------------------------------------------------------------------ 1. axpy against the host path, bit for bit
@pytest.mark.parametrize("kind", ["overlap", "subset", "disjoint", "released", "empty"])
@pytest.mark.parametrize("coeff", COEFFS)
@pytest.mark.parametrize("column", [0, 1])
def test_axpy_equals_vec_add_to(Engine, Snapshot, mols, vecs, column, coeff, kind):
    mol = mols("Ne")
    (da, va), _ = vecs
    db, vb = _b_list(kind, vecs)
    A, T, B = _loaded(Engine, mol, da, va), _loaded(Engine, mol, da, va), _loaded(Engine, mol, db, vb, seed=SEED_B)
    if kind == "released":      # the same compression on both twins: positions are released, the free stack is in use
        for e in (A, T):
            e.compress_vec(300, 0.37)
        assert A.vec_info()[2] > 0, "no released position"
        _same_vectors(A, T)
    size0, _, free0 = A.vec_info()
    with Snapshot([B]) as sb:
        ld, lv = sb.vector()
        assert ld.tobytes() == db.tobytes() and lv.tobytes() == vb.tobytes()
        prod = coeff * lv
        n_nonz = int(np.count_nonzero(prod))
        n0 = A.kernel_launches
        n_taken = A.axpy_snapshot(column, coeff, sb)
        if kind == "empty":
            assert A.kernel_launches == n0          # returns at once
    T.vec_add_to(column, ld, prod, np.ones(ld.size, dtype=np.uint8))
    print(f"column {column} coeff {coeff!r} {kind}: {ld.size} entries, {n_nonz} non-zero products, n_taken {n_taken}; size {size0} -> {A.vec_info()[0]}, free {free0} -> {A.vec_info()[2]}")
    assert n_taken == n_nonz
    _same_vectors(A, T)
    size1, _, free1 = A.vec_info()
    if kind == "subset":
        assert (size1, free1) == (size0, free0)                     # no insert
    if kind == "disjoint" and n_nonz:
        assert size1 - size0 + (free0 - free1) == n_nonz            # only inserts
    if kind == "released" and n_nonz:
        assert free1 < free0                                        # the free stack is used
    if kind == "overlap" and coeff == 1.0:
        assert 0 < size1 - size0 < n_nonz
    for e in (A, T, B):
        e.close()


def test_axpy_with_every_product_zero(Engine, Snapshot, mols, vecs):
    """2**-1074 times a value of magnitude <= 1/2 rounds to zero: nothing is merged and the vector keeps its bytes"""
    mol = mols("Ne")
    (da, va), (db, vb) = vecs
    tiny = vb * (0.5 / np.abs(vb).max())
    assert not np.any(2.0 ** -1074 * tiny) and np.all(tiny != 0)
    A, B = _loaded(Engine, mol, da, va), _loaded(Engine, mol, db, tiny, seed=SEED_B)
    before = A.vector()[1].tobytes(), _column(A, 1).tobytes(), A.vec_info()
    with Snapshot([B]) as sb:
        for column in (0, 1):
            assert A.axpy_snapshot(column, 2.0 ** -1074, sb) == 0
            n0 = A.kernel_launches
            assert A.axpy_snapshot(column, 0.0, sb) == 0 and A.kernel_launches == n0        # coeff == 0: no launch
    assert (A.vector()[1].tobytes(), _column(A, 1).tobytes(), A.vec_info()) == before
    A.close()
    B.close()


# ------------------------------------------------------------------ 2. chunks
def _random_ne_dets(mol, n, seed):
    rng = np.random.RandomState(seed)
    half = mol.n_elec // 2
    out = set()
    while len(out) < n:
        d = 0
        for spin in (0, 1):
            for p in rng.choice(mol.n_orb, half, replace=False):
                d |= 1 << (int(p) + spin * mol.n_orb)
        out.add(d)
    return np.array(sorted(out), dtype=np.uint64)[rng.permutation(n)]


@pytest.mark.parametrize("n_entries", [5097, 11000])
@pytest.mark.parametrize("column", [0, 1])
def test_axpy_in_chunks(Engine, Snapshot, mols, vecs, column, n_entries):
    """vec_nonz = 6000, mat_nonz = 1000: the spawn buffers hold mat_nonz + 4096 = 5096 entries.  5097 entries: the capacity plus one
    (chunks of 5096 and 1); 11000: three chunks, the cuts at odd multiples of 8 bytes as well as even ones."""
    mol = mols("Ne")
    par = dict(NE, vec_nonz=6000, mat_nonz=1000, max_dets=40000)
    cap = par["mat_nonz"] + 4096
    assert n_entries >= cap + 1
    (da, va), _ = vecs
    db = _random_ne_dets(mol, n_entries, 7)
    db[:da.size // 2] = da[:da.size // 2]          # some are stored already
    assert np.unique(db).size == n_entries
    vb = np.random.RandomState(8).standard_normal(n_entries)
    A, T, B = _loaded(Engine, mol, da, va, par), _loaded(Engine, mol, da, va, par), _loaded(Engine, mol, db, vb, par)
    with Snapshot([B]) as sb:
        ld, lv = sb.vector()
        assert sb.info.n_entries == n_entries > cap
        n_taken = A.axpy_snapshot(column, -0.37, sb)
    with pytest.raises(RuntimeError, match="Too many elements"):       # the host path takes no more than the capacity at once
        T.vec_add_to(column, ld[:cap + 1], lv[:cap + 1], np.ones(cap + 1, dtype=np.uint8))
    for k in range(0, n_entries, cap):          # the twin is fed the same slices
        T.vec_add_to(column, ld[k:k + cap], -0.37 * lv[k:k + cap], np.ones(ld[k:k + cap].size, dtype=np.uint8))
    assert n_taken == n_entries
    _same_vectors(A, T)
    assert A.vec_info()[0] == da.size + n_entries - da.size // 2
    for e in (A, T, B):
        e.close()


# ------------------------------------------------------------------ 3. over ranks
@pytest.mark.parametrize("P", [2, 3])
@pytest.mark.parametrize("column", [0, 1])
def test_axpy_over_ranks(Engine, Snapshot, mols, vecs, P, column):
    mol = mols("Ne")
    _, (db, vb) = vecs
    coeff = -0.37
    S = Sharded(Engine, mol, P, SEED_A, NE, n_iter=5)
    lists = [_live(e) for e in S.eng]
    ud, uv = np.concatenate([d for d, _ in lists]), np.concatenate([v for _, v in lists])
    assert np.unique(ud).size == ud.size and all(d.size for d, _ in lists)
    # b and, behind it, 1500 determinants no shard holds yet: the shards look up and insert
    extra = _random_ne_dets(mol, 1500, 5)
    extra = extra[~np.isin(extra, ud) & ~np.isin(extra, db)]
    db, vb = np.concatenate([db, extra]), np.concatenate([vb, np.random.RandomState(6).standard_normal(extra.size)])
    assert extra.size > 1000
    one, B = _loaded(Engine, mol, ud, uv), _loaded(Engine, mol, db, vb, seed=SEED_B)
    taken = [None] * P
    with Snapshot([B]) as sb:
        n_one = one.axpy_snapshot(column, coeff, sb)

        def job(k):
            def run():
                taken[k] = S.eng[k].axpy_snapshot(column, coeff, sb)
            return run
        _threads([job(k) for k in range(P)])
    assert sum(taken) == n_one == int(np.count_nonzero(coeff * vb)) and all(t > 0 for t in taken), taken
    union = {}
    for k, e in enumerate(S.eng):
        d = e.vector()[0]
        v0, v1 = e.vector()[1], _column(e, 1)
        stored = (v0 != 0) | (v1 != 0)
        assert np.all(e.idx_to_proc(d[stored]) == k), f"a determinant on shard {k} that idx_to_proc names for another"
        col = v1 if column else v0
        for x, y in zip(d[col != 0], col[col != 0]):
            assert int(x) not in union
            union[int(x)] = float(y).hex()
    od = one.vector()[0]
    oc = _column(one, column)
    want = {int(x): float(y).hex() for x, y in zip(od[oc != 0], oc[oc != 0])}
    print(f"P={P} column {column}: taken per shard {taken}; {len(union)} non-zero elements in the union")
    assert union == want
    for x in (S, one, B):
        x.close()


# ------------------------------------------------------------------ 4. snapshot_dot
def _dot_ref(da, va, db, vb):
    b = {int(d): float(v) for d, v in zip(db, vb) if v != 0}
    prods = [float(v) * b[int(d)] for d, v in zip(da, va) if v != 0 and int(d) in b]
    return dict(dot=math.fsum(prods), abs_sum=math.fsum(abs(p) for p in prods), n_src=int(np.count_nonzero(va)), n_hits=len(prods))


def _check_dot(tag, got, ref):
    bound = (ref["n_hits"] + 8) * U * ref["abs_sum"]
    print(f"{tag}: dot {got.dot!r} ref {ref['dot']!r} err {abs(got.dot - ref['dot']):.3e} bound {bound:.3e}; n_src {got.n_src} n_hits {got.n_hits}")
    assert (got.n_src, got.n_hits) == (ref["n_src"], ref["n_hits"])
    assert abs(got.dot - ref["dot"]) <= bound and abs(got.abs_sum - ref["abs_sum"]) <= bound
    return bound


def test_snapshot_dot(Engine, Snapshot, mols, vecs):
    mol = mols("Ne")
    (da, va), (db, vb) = vecs
    va = va.copy()
    va[::41] = 0.0                      # stored positions without a value: visited by no one
    ea, eb = _loaded(Engine, mol, da, va), _loaded(Engine, mol, db, vb, seed=SEED_B)
    with Snapshot([eb]) as sb, Snapshot([ea]) as sa:
        ab = sb.dot([ea])
        bound_ab = _check_dot("(a, b)", ab, _dot_ref(da, va, db, vb))
        assert ab.n_hits > 0
        ba = sa.dot([eb])
        bound_ba = _check_dot("(b, a)", ba, _dot_ref(db, vb, da, va))
        assert ab.n_hits == ba.n_hits and abs(ab.dot - ba.dot) <= bound_ab + bound_ba
        hd = ea.h_dot(eb)               # the overlap fries_h_dot forms of the same products in its own order
        assert abs(ab.dot - hd.ovlp) <= 2 * bound_ab
        for _ in range(2):
            assert sb.dot([ea]) == ab   # the same bits
        aa = sa.dot([ea])
        ref_aa = _dot_ref(da, va, da, va)
        assert ref_aa["dot"] == math.fsum(float(x) * float(x) for x in va) and ref_aa["n_hits"] == ref_aa["n_src"]
        _check_dot("(a, a)", aa, ref_aa)
        # column 1: b's list added into it, then dotted with b
        ea.axpy_snapshot(1, 1.0, sb)
        c1 = _column(ea, 1)
        _check_dot("column 1", sb.dot([ea], column=1), _dot_ref(ea.vector()[0], c1, db, vb))
    ea.close()
    eb.close()


@pytest.mark.parametrize("P", [2, 3])
def test_snapshot_dot_over_shards(Engine, Snapshot, mols, vecs, P):
    mol = mols("Ne")
    _, (db, vb) = vecs
    S = Sharded(Engine, mol, P, SEED_A, NE, n_iter=5)
    lists = [_live(e) for e in S.eng]
    ud, uv = np.concatenate([d for d, _ in lists]), np.concatenate([v for _, v in lists])
    one, B = _loaded(Engine, mol, ud, uv), _loaded(Engine, mol, db, vb, seed=SEED_B)
    with Snapshot([B]) as sb:
        got, whole = sb.dot(S.eng), sb.dot([one])
        ref = _dot_ref(ud, uv, db, vb)
        bound = _check_dot(f"P={P}", got, ref)
        _check_dot("the union", whole, ref)
        assert (got.n_src, got.n_hits) == (whole.n_src, whole.n_hits) and abs(got.dot - whole.dot) <= 2 * bound
        assert sb.dot(S.eng) == got
    for x in (S, one, B):
        x.close()


# ------------------------------------------------------------------ 5. scale and one_norm
@pytest.mark.parametrize("drop", [0, 1])
def test_scale_and_one_norm(Engine, Snapshot, mols, vecs, drop):
    """drop = 1: one position less, so that both an even and an odd size are scaled"""
    mol = mols("Ne")
    (da, va), (db, vb) = vecs
    da, va = da[:da.size - drop], va[:va.size - drop]
    e, B = _loaded(Engine, mol, da, va), _loaded(Engine, mol, db, vb, seed=SEED_B)
    with Snapshot([B]) as sb:
        e.axpy_snapshot(1, 1.0, sb)
    d = e.vector()[0]
    v0, v1 = e.vector()[1], _column(e, 1)
    assert np.count_nonzero(v1) == vb.size and v0.size >= da.size
    norm = e.one_norm()
    assert norm == e.one_norm(0) == e.find_preserve(NE["vec_nonz"])[1]
    assert abs(norm - math.fsum(np.abs(v0))) <= (v0.size + 8) * U * norm
    x = _loaded(Engine, mol, d, v1)         # column 1's values as another engine's column 0: the same sum in the same order
    assert e.one_norm(1) == x.one_norm(0) == x.find_preserve(NE["vec_nonz"])[1]
    for col, f, want in ((0, -0.37, v0 * -0.37), (1, 1.0 / 3.0, v1 * (1.0 / 3.0))):
        other = _column(e, 1 - col).tobytes()
        e.scale(col, f)
        assert _column(e, col).tobytes() == want.tobytes() and _column(e, 1 - col).tobytes() == other
    assert e.vector()[0].tobytes() == d.tobytes()
    for y in (e, B, x):
        y.close()


def test_one_norm_over_two_ranks(Engine, mols):
    S = Sharded(Engine, mols("Ne"), 2, SEED_A, NE, n_iter=5)
    vals = np.concatenate([e.vector()[1] for e in S.eng])
    got = [None, None]

    def job(k):
        def run():
            got[k] = S.eng[k].one_norm(0)
        return run
    _threads([job(0), job(1)])
    ref = math.fsum(np.abs(vals))
    print(f"one-norm over 2 ranks {got[0]!r}, fsum {ref!r}")
    assert got[0] == got[1] and abs(got[0] - ref) <= (vals.size + 8) * U * ref
    S.close()


# ------------------------------------------------------------------ 6. refusals
def _refused(call, who, engines, match):
    n0 = [e.kernel_launches for e in engines]
    with pytest.raises(RuntimeError, match=match) as ex:
        call()
    assert who in str(ex.value), str(ex.value)
    assert [e.kernel_launches for e in engines] == n0


def _raw(lib, name, *args):
    rc = getattr(lib, name)(*args)
    return rc, lib.fries_last_error().decode()


def _hh(Engine):
    hh_run = golden_io.manifest()["hh_runs"]["hh_l6_m2000"]
    hh = Engine(None)
    hh.setup_hh(vec_nonz=100, max_dets=1000, **{k: hh_run[k] for k in ("n_elec", "n_sites", "eps", "U", "omega", "g", "gs_energy", "target_norm", "initiator", "seed")})
    return hh


def test_refusals_launch_nothing(Engine, Snapshot, mols):
    from fries_amd.engine import VdotResult, _handles
    mol = mols("Ne")
    plain = Engine(mol)
    plain.setup(**SMALL)
    lib = plain.lib
    snap = Snapshot([plain])
    n_taken, res, norm = C.c_uint64(), VdotResult(), C.c_double()
    _, one = _handles([plain])
    calls = {
        "fries_vec_axpy_snapshot": lambda e, column=0, sn=None: e.axpy_snapshot(column, 1.0, sn if sn is not None else snap),
        "fries_snapshot_dot": lambda e, column=0, sn=None: (sn if sn is not None else snap).dot([e], column),
        "fries_vec_scale": lambda e, column=0, sn=None: e.scale(column, 2.0),
        "fries_vec_one_norm": lambda e, column=0, sn=None: e.one_norm(column),
    }
    # null arguments
    n0 = plain.kernel_launches
    null_args = {
        "fries_vec_axpy_snapshot": [(None, 0, 1.0, snap.h, C.byref(n_taken)), (plain.h, 0, 1.0, None, C.byref(n_taken)), (plain.h, 0, 1.0, snap.h, None)],
        "fries_snapshot_dot": [(None, 1, 0, snap.h, C.byref(res)), ((C.c_void_p * 1)(None), 1, 0, snap.h, C.byref(res)), (one, 1, 0, None, C.byref(res)), (one, 1, 0, snap.h, None)],
        "fries_vec_scale": [(None, 0, 2.0)],
        "fries_vec_one_norm": [(None, 0, C.byref(norm)), (plain.h, 0, None)],
    }
    for who, arg_lists in null_args.items():
        for args in arg_lists:
            rc, msg = _raw(lib, who, *args)
            assert rc != 0 and f"{who}: null argument" in msg, (who, msg)
    assert plain.kernel_launches == n0
    hh, empty, bare = _hh(Engine), Engine(None), Engine(mol)
    other = Engine(mols("H2O"))
    other.setup(**SMALL)
    relabelled = Engine(dataclasses.replace(mol, irreps=np.zeros_like(mol.irreps)))
    relabelled.setup(**SMALL)
    flipped = Engine(mol)
    flipped.setup(**SMALL)
    flipped.set_spin_parity(1)
    with Snapshot([other]) as so, Snapshot([relabelled]) as sr, Snapshot([flipped]) as sf:
        for who, call in calls.items():
            # a Hubbard-Holstein context; no molecule; no solution vector; a column other than 0 or 1
            _refused(lambda: call(hh), who, [hh], "Hubbard-Holstein")
            _refused(lambda: call(empty), who, [empty], "fries_set_molecule")
            _refused(lambda: call(bare), who, [bare], "solution vector")
            for column in (2, -1):
                _refused(lambda: call(plain, column), who, [plain], "column must be 0 or 1")
            if "snapshot" not in who:
                continue
            # a snapshot of another molecule (shape; irreps) or spin_parity, from either side
            _refused(lambda: call(plain, 0, so), who, [plain], "different molecules")
            _refused(lambda: call(other, 0, snap), who, [other], "different molecules")
            _refused(lambda: call(plain, 0, sr), who, [plain], "irreps")
            _refused(lambda: call(relabelled, 0, snap), who, [relabelled], "irreps")
            _refused(lambda: call(plain, 0, sf), who, [plain], "spin_parity")
            _refused(lambda: call(flipped, 0, snap), who, [flipped], "spin_parity")
            # a snapshot on another device than the context: reachable where a second device is visible
            if lib.fries_device_count() > 1:
                far = Engine(mol, device=1)
                far.setup(**SMALL)
                with Snapshot([far]) as sfar:
                    assert sfar.info.device == 1
                    _refused(lambda: call(plain, 0, sfar), who, [plain], "different devices")
                far.close()
            else:
                print(f"{who}: one device visible, the refusal of a snapshot on another device cannot be reached here")
    # `a` of fries_snapshot_dot follows the completeness rule of fries_h_dot_ranks
    A = Sharded(Engine, mol, 2, 1, SMALL)
    for shards in ([A.eng[0]], [A.eng[1], A.eng[0]], [A.eng[0], A.eng[1], plain]):
        _refused(lambda: snap.dot(shards), "fries_snapshot_dot", A.eng + [plain], "ranks 0 .. P - 1 of one run")
    for n_a in (0, 65):
        rc, msg = _raw(lib, "fries_snapshot_dot", (C.c_void_p * 65)(*[plain.h] * 65), n_a, 0, snap.h, C.byref(res))
        assert rc != 0 and "fries_snapshot_dot" in msg and "between 1 and 64" in msg, msg
    # what is served: one shard of a sharded run takes its own entries; the shards of a run are dotted
    assert sum(e.axpy_snapshot(0, 1.0, snap) for e in A.eng) == 1 and snap.dot(A.eng).n_hits == 1
    snap.close()
    for x in (A, hh, empty, bare, other, relabelled, flipped, plain):
        x.close()
