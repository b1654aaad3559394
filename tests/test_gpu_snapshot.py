"""-m gpu: vector snapshots (csrc/snapshot.hip) and the estimators over ranks built on them: fries_snapshot_*, fries_h_dot_ranks,
fries_rdm1_ranks, fries_rdm2_ranks, VecSnapshot and FriReplicas(ranks=...).

The setup is the Ne shape at pair_common.NE_PAIR, seeds 1 and 2, 25 iterations: unsharded (pair_common.ne_pair) and with P = 2 and 3
rank threads over the native local transport, as test_gpu_pins._rank_thread_run drives them.

Bounds.  Sharding changes the order in which the same terms are added, nothing else.  u = 2**-53 throughout.
  * fries_h_dot_ranks against the host reference of test_gpu_hdot (fsum over the terms): (N + 8) u abs_ref, that module's bound, which
    holds for ANY association order of the N terms.
  * every bin of gamma and gamma2 against the one-rank call on the union of the shards: both results add the same rounded products in
    some order, so each is within (n + 8) u S of the exact sum of the bin (n terms of summed magnitude S; the references of test_gpu_rdm1 /
    test_gpu_rdm2 give n and S per bin), and they differ by at most twice that.  It is the bound test_gpu_rdm2.test_several_chunks uses
    for its other association order.  A worst case, not a measurement.
The counts are integers and must be equal."""
import ctypes as C
import dataclasses
import math
import threading

import numpy as np
import pytest

import golden_io
import pair_common as pc
import test_gpu_hdot as th
import test_gpu_rdm1 as t1
import test_gpu_rdm2 as t2
from fries_amd import fcidump
from pair_common import NE_PAIR, SMALL, U, as_map, same_bits

pytestmark = pytest.mark.gpu
KINDS = ("h_dot", "rdm1", "rdm2")


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
    """One frisys_mol run over P rank threads of this process (LocalGroup); the engines stay open"""

    def __init__(self, Engine, mol, P, seed, par=NE_PAIR, n_iter=0):
        from fries_amd.comm import LocalGroup
        par = {k: v for k, v in par.items() if k != "seed"}        # (the seed is this class's own argument)
        self.grp = LocalGroup(P, par["mat_nonz"])
        self.eng = [Engine(mol, device=0, comm=self.grp.comm(k, 0)) for k in range(P)]
        _threads([(lambda e=e: e.setup(seed=seed, **par)) for e in self.eng])
        self.logs = [[] for _ in range(P)]
        if n_iter:
            self.iterate(n_iter)

    def iterate(self, k):
        def job(j):
            return lambda: self.logs[j].append(self.eng[j].iterate(k))
        _threads([job(j) for j in range(len(self.eng))])

    def log_bytes(self):
        return [np.concatenate(lg).tobytes() for lg in self.logs]

    def vectors(self):
        return [e.vector() for e in self.eng]

    def live(self):
        """the shards' live entries, rank-major and in position order: what a snapshot holds"""
        ds, vs = zip(*self.vectors())
        d, v = np.concatenate(ds), np.concatenate(vs)
        return d[v != 0], v[v != 0]

    def close(self):
        for e in self.eng:
            e.close()
        self.grp.destroy()


def _all_three(snap, a):
    return snap.h_dot(a), snap.rdm1(a), snap.rdm2(a)


def _direct(a, b):
    return a.h_dot(b), a.rdm1(b), a.rdm2(b)


def _same(x, y):
    return x[0] == y[0] and same_bits(x[1], y[1]) and same_bits(x[2], y[2])


def _launches(engines):
    return [e.kernel_launches for e in engines]


# ------------------------------------------------------------------ 1. one shard gives the same bits
@pytest.mark.parametrize("pair", ["ne", "min4"])
def test_one_shard_gives_the_same_bits(Engine, Snapshot, mols, pair):
    if pair == "ne":
        ea, eb = pc.ne_pair(Engine, mols("Ne"))
    else:
        ea, eb = pc.min4_pair(Engine, mols("MIN4"), 20261)[:2]
    with Snapshot([eb]) as sb, Snapshot([ea]) as sa:
        assert sb.info.n_shards == 1 and sb.info.n_entries == int((eb.vector()[1] != 0).sum()) and sb.info.device == 0
        want_ab, want_aa = _direct(ea, eb), _direct(ea, ea)
        got_ab, got_aa = _all_three(sb, [ea]), _all_three(sa, [ea])
        assert got_ab[0].n_hits > 0 and got_ab[2].n_hits > 0
        assert _same(got_ab, want_ab), pair
        assert _same(got_aa, want_aa), pair
        for _ in range(2):
            assert _same(_all_three(sb, [ea]), got_ab) and _same(_all_three(sa, [ea]), got_aa)
        assert _same(_direct(ea, eb), want_ab)
    for e in (ea, eb):
        e.close()


# ------------------------------------------------------------------ 2. sharded against the union
@pytest.fixture(scope="module", params=[2, 3])
def sharded_pair(request, Engine, mols):
    """Seeds 1 and 2 over P ranks, 25 iterations; the unions of the shards in two plain engines; the host references, computed once"""
    P = request.param
    mol = mols("Ne")
    A, B = Sharded(Engine, mol, P, 1, n_iter=25), Sharded(Engine, mol, P, 2, n_iter=25)
    ua, ub, eh = Engine(mol), Engine(mol), Engine(mol)
    for e in (ua, ub, eh):
        e.setup(seed=1, **NE_PAIR)
    (da, va), (db, vb) = A.live(), B.live()
    ua.vec_load(da, va)
    ub.vec_load(db, vb)
    a, b = as_map(da, va), as_map(db, vb)
    assert len(a) == da.size and len(b) == db.size          # the shards are disjoint
    cols, diag = th._dense(eh, set(a) | set(b))
    ref = dict(hd=th._reference(a, b, cols, diag), hd_ba=th._reference(b, a, cols, diag), r1=t1._reference(a, b, mol.n_orb), r2=t2._reference(a, b, mol.n_orb))
    yield dict(P=P, mol=mol, A=A, B=B, ua=ua, ub=ub, ref=ref)
    for x in (A, B, ua, ub, eh):
        x.close()


def test_sharded_against_the_union(sharded_pair, Snapshot):
    s = sharded_pair
    mol, A, B, ua, ub, ref = s["mol"], s["A"], s["B"], s["ua"], s["ub"], s["ref"]
    n, n_elec = mol.n_orb, mol.n_elec
    assert all(e.vec_info()[1] > 0 for e in A.eng + B.eng), "an empty shard after 25 iterations"
    one_hd, one_r1, one_r2 = _direct(ua, ub)
    with Snapshot(B.eng) as sb, Snapshot(A.eng) as sa:
        assert sb.info.n_shards == s["P"] and sb.info.n_entries == ub.vec_info()[1]
        hd, r1, r2 = _all_three(sb, A.eng)
        hd_ba, r1_ba, r2_ba = _all_three(sa, B.eng)
    # the counts are those of the one-rank calls
    for got, one in ((hd, one_hd), (r1, one_r1), (r2, one_r2)):
        assert (got.n_src, got.n_terms, got.n_hits) == (one.n_src, one.n_terms, one.n_hits)
    assert hd.n_hits > 0 and r2.n_hits > 0
    # h, ovlp, abs_sum against the host's fsum: (N + 8) u abs_ref (asserted by test_gpu_hdot._check, with the counts)
    bound_h = th._check(f"P={s['P']} (a,b)", hd, ref["hd"])
    th._check(f"P={s['P']} (b,a)", hd_ba, ref["hd_ba"])
    # every bin against the one-rank matrices: twice the bin's (n + 8) u S (module docstring)
    for tag, got, one, bound in (("gamma", r1.gamma, one_r1.gamma, ref["r1"]["bound"]), ("gamma2", r2.gamma2, one_r2.gamma2, ref["r2"]["bound"])):
        err = np.abs(got - one)
        worst = np.unravel_index(np.argmax(err - 2 * bound), err.shape)
        print(f"P={s['P']} {tag}: {int((got != 0).sum())} non-zero bins, {int((err != 0).sum())} differ from the one-rank call; worst {worst}: err {err[worst]:.3e} bound {2 * bound[worst]:.3e}")
        assert np.all(err <= 2 * bound), tag
    for got, one, r in ((r1, one_r1, ref["r1"]), (r2, one_r2, ref["r2"])):
        assert abs(got.ovlp - one.ovlp) <= 2 * r["bound_ov"] and abs(got.abs_sum - one.abs_sum) <= 2 * r["bound_abs"]
    t1._check("rdm1 over ranks", r1, ref["r1"])
    t1._check_gamma("rdm1 over ranks", r1.gamma, ref["r1"])
    t2._check("rdm2 over ranks", r2, ref["r2"])
    t2._check_gamma("rdm2 over ranks", r2.gamma2, ref["r2"])
    # the identities of DESIGN.md 6g on the sharded result, with the allowances of test_gpu_rdm2.test_ties_to_rdm1_and_h_dot
    assert np.array_equal(r2.gamma2, r2.gamma2.transpose(2, 3, 0, 1))          # bit for bit
    t2._check_full_trace("rdm2 over ranks", r2, ref["r2"], n_elec)
    t1._check_trace("rdm1 over ranks", r1, ref["r1"], n_elec)
    pt = np.einsum("pqrr->pq", r2.gamma2)
    allow = np.einsum("pqrr->pq", ref["r2"]["bound"]) + (n_elec - 1) * ref["r1"]["bound"] + 4 * U * (np.einsum("pqrr->pq", np.abs(r2.gamma2)) + (n_elec - 1) * np.abs(r1.gamma))
    assert np.all(np.abs(pt - (n_elec - 1) * r1.gamma) <= allow) and np.any(pt != 0)
    h_core, eri4 = np.asarray(mol.h_core), t2._eri4(mol)
    p1, p2 = (h_core * r1.gamma).ravel(), (0.5 * eri4 * r2.gamma2).ravel()
    got, want = math.fsum(p1) + math.fsum(p2), hd.h + ua.hf_energy * hd.ovlp
    allow_e = ((hd.n_hits + hd.n_src + 8) * U * hd.abs_sum + float(np.sum(np.abs(h_core) * ref["r1"]["bound"])) + 0.5 * float(np.sum(np.abs(eri4) * ref["r2"]["bound"]))
               + 4 * U * (float(np.sum(np.abs(p1))) + float(np.sum(np.abs(p2))) + abs(ua.hf_energy * hd.ovlp) + abs(hd.h)))
    print(f"P={s['P']}: sum(h gamma) + 1/2 sum(eri Gamma) {got!r}; h + hf_en * ovlp {want!r}; difference {abs(got - want):.3e}; allowance {allow_e:.3e}")
    assert abs(got - want) <= allow_e
    # swapping the replicas: H is symmetric, the matrices are each other's transposes -- the same products from the other side
    assert abs(hd.h - hd_ba.h) <= bound_h and abs(hd.ovlp - hd_ba.ovlp) <= 2 * ref["r1"]["bound_ov"]
    assert np.all(np.abs(r1.gamma - r1_ba.gamma.T) <= 2 * ref["r1"]["bound"])
    assert np.all(np.abs(r2.gamma2 - r2_ba.transposed().gamma2) <= 2 * ref["r2"]["bound"])
    t1._check_gamma("rdm1 (b,a)", r1_ba.gamma, ref["r1"], transposed=True)
    t2._check_gamma("rdm2 (b,a)", r2_ba.gamma2, ref["r2"], transposed=True)


def test_rdm2_record_capacity_over_ranks(sharded_pair, Engine, Snapshot, monkeypatch):
    """fries_rdm2_ranks under a small FRIES_RDM2_RECORDS (read when a context is created), as test_gpu_rdm2.test_several_chunks does for
    fries_rdm2.  The capacity is the largest need of one workgroup (R2_BPOS positions) of any shard, from the records the host reference
    counts per source: the shards then need several chunks, another association order within the same bound.  One record less and the
    call is refused -- after every shard's counting pass, the launches that tell the need, and before any record is written: one launch
    per shard, gamma2 and the result left zero."""
    from fries_amd.engine import Rdm2Result, _handles
    s = sharded_pair
    P, mol, A, B, ref = s["P"], s["mol"], s["A"], s["B"], s["ref"]["r2"]
    shard_wg = [[sum(ref["rec"].get(int(x), 0) for x, y in zip(d[k:k + t2.R2_BPOS], v[k:k + t2.R2_BPOS]) if y != 0) for k in range(0, d.size, t2.R2_BPOS)] for d, v in A.vectors()]
    cap = max(max(w) for w in shard_wg)
    chunks = [t2._cut(w, cap) for w in shard_wg]
    print(f"P={P}: records per workgroup {shard_wg}; capacity {cap}: chunks per shard {chunks}")
    assert sum(len(c) for c in chunks) > P          # several chunks in at least one shard
    monkeypatch.setenv("FRIES_RDM2_RECORDS", str(cap))
    C_ = Sharded(Engine, mol, P, 1, n_iter=25)
    monkeypatch.setenv("FRIES_RDM2_RECORDS", str(cap - 1))
    T = Sharded(Engine, mol, P, 1, n_iter=25)
    monkeypatch.delenv("FRIES_RDM2_RECORDS")
    for X in (C_, T):
        assert all(x.tobytes() == y.tobytes() for (dx, vx), (dy, vy) in zip(X.vectors(), A.vectors()) for x, y in ((dx, dy), (vx, vy)))
    with Snapshot(B.eng) as sb:
        whole = sb.rdm2(A.eng)
        n0 = _launches(C_.eng)
        chunked = sb.rdm2(C_.eng)
        # per shard the counting pass, then per chunk the emitting pass, three launches per 8-bit pass of the sort (22^4 bins: 3 passes) and the two of the sum
        assert [x - y for x, y in zip(_launches(C_.eng), n0)] == [1 + len(c) * (1 + 3 * 3 + 2) for c in chunks]
        t2._check("chunked over ranks", chunked, ref)
        t2._check_gamma("chunked over ranks", chunked.gamma2, ref)
        assert np.all(np.abs(chunked.gamma2 - whole.gamma2) <= 2 * ref["bound"]) and chunked[1:] == whole[1:]
        assert np.array_equal(chunked.gamma2, chunked.gamma2.transpose(2, 3, 0, 1))
        assert same_bits(sb.rdm2(C_.eng), chunked)
        # one record less: refused
        n0, nb = _launches(T.eng), _launches(B.eng)
        with pytest.raises(RuntimeError, match="FRIES_RDM2_RECORDS") as ex:
            sb.rdm2(T.eng)
        print(ex.value)
        msg = str(ex.value)
        assert "fries_rdm2_ranks" in msg and "of shard" in msg and str(cap) in msg and str(cap - 1) in msg
        assert [x - y for x, y in zip(_launches(T.eng), n0)] == [1] * P and _launches(B.eng) == nb
        # what the outputs hold after the refusal: zeros
        _, arr = _handles(T.eng)
        g = np.full((mol.n_orb,) * 4, 7.0)
        r = Rdm2Result(1.0, 1.0, 1, 1, 1)
        assert sb.lib.fries_rdm2_ranks(arr, P, sb.h, g.ctypes.data_as(C.c_void_p), C.byref(r)) != 0
        assert not g.any() and (r.ovlp, r.abs_sum, r.n_src, r.n_terms, r.n_hits) == (0.0, 0.0, 0, 0, 0)
    C_.close()
    T.close()


# ------------------------------------------------------------------ 3. edges
def test_snapshot_straight_after_setup(Engine, Snapshot, mols):
    """P = 3 right after the set-up: the Hartree-Fock determinant sits on one rank, the other two shards are empty"""
    mol = mols("Ne")
    A = Sharded(Engine, mol, 3, 1)
    plain = Engine(mol)
    plain.setup(seed=1, **NE_PAIR)
    assert sorted(e.vec_info()[1] for e in A.eng) == [0, 0, 1]
    empty = [e for e in A.eng if e.vec_info()[0] == 0]
    n0 = _launches(empty)
    with Snapshot(A.eng) as sn:
        assert sn.info.n_entries == 1 and sn.info.n_shards == 3 and sn.info.n_slots == 1 << 14
        d, v = sn.vector()
        pd, pv = plain.vector()
        assert d.tobytes() == pd[pv != 0].tobytes() and v.tobytes() == pv[pv != 0].tobytes()
        got = _all_three(sn, A.eng)
        assert _same(got, _direct(plain, plain))           # one term per sum: no order to differ in
        assert got[0].n_src == 1 and got[0].ovlp == float(v[0]) ** 2
        assert _same(_all_three(sn, [plain]), got)
    assert _launches(empty) == n0                          # an empty shard launches nothing
    A.close()
    plain.close()


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


def test_table_larger_than_the_minimum(Engine, Snapshot, mols):
    """7000 determinants: more than 2^14 slots hold at 40 % fill (6553), so the snapshot's table has 2^15"""
    mol = mols("Ne")
    e = Engine(mol)
    e.setup(seed=1, **dict(NE_PAIR, max_dets=8000))
    dets = _random_ne_dets(mol, 7000, 99)
    vals = np.random.RandomState(100).standard_normal(7000)
    vals[::97] = 0.0
    e.vec_load(dets, vals)
    with Snapshot([e]) as sn:
        info = sn.info
        print(info)
        assert (info.ms_compact, info.ms_copy, info.ms_insert) == (0.0, 0.0, 0.0)      # timed under FRIES_SNAPSHOT_EVENTS=1 only
        assert info.n_entries == int((vals != 0).sum()) and info.n_slots == 1 << 15 and info.device_bytes >= 16 * info.n_slots + 16 * 7000
        d, v = sn.vector()
        assert d.tobytes() == dets[vals != 0].tobytes() and v.tobytes() == vals[vals != 0].tobytes()
        got, want = _all_three(sn, [e]), _direct(e, e)
        assert want[0].n_src == info.n_entries and want[0].n_hits > 0 and want[2].n_hits > 0
        assert _same(got, want)
    e.close()


def test_snapshot_vector_is_rank_major_in_position_order(sharded_pair, Snapshot):
    B = sharded_pair["B"]
    want_d, want_v = B.live()
    with Snapshot(B.eng) as sn:
        d, v = sn.vector()
        cap_short = C.c_uint64()
        rc = sn.lib.fries_snapshot_vector(sn.h, None, None, 1, C.byref(cap_short))
        assert rc != 0 and "fries_snapshot_vector" in sn.lib.fries_last_error().decode() and cap_short.value == want_d.size
    assert d.tobytes() == want_d.tobytes() and v.tobytes() == want_v.tobytes()


# ------------------------------------------------------------------ 4. the snapshot is frozen
def test_the_snapshot_is_frozen(Engine, Snapshot, mols):
    mol = mols("Ne")
    A, B = Sharded(Engine, mol, 2, 1, n_iter=25), Sharded(Engine, mol, 2, 2, n_iter=25)
    with Snapshot(B.eng) as sb:
        before, vec_before = _all_three(sb, A.eng), sb.vector()
        old = B.live()
        B.iterate(5)
        assert B.live()[1].tobytes() != old[1].tobytes()
        assert _same(_all_three(sb, A.eng), before)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(sb.vector(), vec_before))
        with Snapshot(B.eng) as later:
            assert later.h_dot(A.eng) != before[0]
        for e in B.eng:     # the snapshot outlives its source
            e.close()
        assert _same(_all_three(sb, A.eng), before)
    for e in A.eng:
        e.close()
    A.grp.destroy()
    B.grp.destroy()


# ------------------------------------------------------------------ 5. refusals
def _refused(call, who, engines, match):
    n0 = _launches(engines)
    with pytest.raises(RuntimeError, match=match) as ex:
        call()
    assert who in str(ex.value), str(ex.value)
    assert _launches(engines) == n0


def _raw(lib, name, *args):
    rc = getattr(lib, name)(*args)
    return rc, lib.fries_last_error().decode()


def test_snapshot_create_refusals_launch_nothing(Engine, Snapshot, mols):
    from fries_amd.engine import _handles
    who = "fries_snapshot_create"
    mol = mols("Ne")
    plain = Engine(mol)
    plain.setup(**SMALL)
    lib = plain.lib
    n0 = plain.kernel_launches
    # null arguments; 0 shards and more than FR_MAX_RANKS = 64
    _, one = _handles([plain])
    out = C.c_void_p()
    for args in ((None, one, 1, 0), (C.byref(out), None, 1, 0), (C.byref(out), (C.c_void_p * 1)(None), 1, 0)):
        rc, msg = _raw(lib, who, *args)
        assert rc != 0 and f"{who}: null argument" in msg, msg
    for n_sh in (0, 65):
        rc, msg = _raw(lib, who, C.byref(out), (C.c_void_p * 65)(*[plain.h] * 65), n_sh, 0)
        assert rc != 0 and who in msg and "between 1 and 64" in msg, msg
    assert not out and plain.kernel_launches == n0
    _refused(lambda: Snapshot([plain], device=99), who, [plain], "device index out of range")
    # Hubbard-Holstein; no molecule; no solution vector
    hh_run = golden_io.manifest()["hh_runs"]["hh_l6_m2000"]
    hh = Engine(None)
    hh.setup_hh(vec_nonz=100, max_dets=1000, **{k: hh_run[k] for k in ("n_elec", "n_sites", "eps", "U", "omega", "g", "gs_energy", "target_norm", "initiator", "seed")})
    _refused(lambda: Snapshot([hh]), who, [hh], "Hubbard-Holstein")
    hh.close()
    empty, bare = Engine(None), Engine(mol)
    _refused(lambda: Snapshot([empty]), who, [empty], "fries_set_molecule")
    _refused(lambda: Snapshot([bare]), who, [bare], "solution vector")
    empty.close()
    bare.close()
    # incomplete and mis-ordered shard lists from a P = 2 group; a plain engine is one shard of one
    A = Sharded(Engine, mol, 2, 1, par=SMALL)
    for shards in ([A.eng[0]], [A.eng[1]], [A.eng[1], A.eng[0]], [A.eng[0], A.eng[0]], [A.eng[0], A.eng[1], plain], [plain, plain], [plain, A.eng[1]]):
        _refused(lambda: Snapshot(shards), who, A.eng + [plain], "ranks 0 .. P - 1 of one run")
    # mixed runs: two groups with different seeds
    B = Sharded(Engine, mol, 2, 2, par=SMALL)
    _refused(lambda: Snapshot([A.eng[0], B.eng[1]]), who, A.eng + B.eng, "different runs")
    # shards that differ in molecule, hf_en or spin_parity: groups with the seed of A (the same scramblers where the shape is the same)
    W = Sharded(Engine, mols("H2O"), 2, 1, par=SMALL)
    _refused(lambda: Snapshot([A.eng[0], W.eng[1]]), who, A.eng + W.eng, "different molecules")
    R = Sharded(Engine, dataclasses.replace(mol, irreps=np.zeros_like(mol.irreps)), 2, 1, par=SMALL)
    _refused(lambda: Snapshot([A.eng[0], R.eng[1]]), who, A.eng + R.eng, "irreps")
    S = Sharded(Engine, fcidump.synthetic("Ne", seed=777), 2, 1, par=SMALL)
    _refused(lambda: Snapshot([A.eng[0], S.eng[1]]), who, A.eng + S.eng, "hf_en")
    # two groups set up alike hold the same shards bit for bit, and pass as one run; once one of them has iterated on they do not
    A2 = Sharded(Engine, mol, 2, 1, par=SMALL)
    with Snapshot([A.eng[0], A2.eng[1]]) as mixed, Snapshot(A.eng) as own:
        assert all(x.tobytes() == y.tobytes() for x, y in zip(mixed.vector(), own.vector()))
    A2.iterate(1)
    _refused(lambda: Snapshot([A.eng[0], A2.eng[1]]), who, A.eng + A2.eng, "iteration counts")
    A2.close()
    A.eng[1].set_spin_parity(1)
    _refused(lambda: Snapshot(A.eng), who, A.eng, "spin_parity")
    A.eng[1].set_spin_parity(0)
    with Snapshot(A.eng) as ok:
        assert ok.info.n_entries == 1
    for x in (A, B, W, R, S, plain):
        x.close()


@pytest.mark.parametrize("kind", KINDS)
def test_ranks_refusals_launch_nothing(Engine, Snapshot, mols, kind):
    from fries_amd.engine import HdotResult, Rdm1Result, _handles
    who = f"fries_{kind}_ranks"
    mol = mols("Ne")
    plain = Engine(mol)
    plain.setup(**SMALL)
    lib = plain.lib
    snap = Snapshot([plain])
    call = lambda sn, a: getattr(sn, kind)(a)
    # null arguments; 0 shards and more than 64
    _, one = _handles([plain])
    buf = np.zeros(mol.n_orb ** 4)
    res = HdotResult() if kind == "h_dot" else Rdm1Result()
    args = [one, 1, snap.h] + ([buf.ctypes.data_as(C.c_void_p)] if kind != "h_dot" else []) + [C.byref(res)]
    n0 = plain.kernel_launches
    for k in [j for j in range(len(args)) if j != 1] + ["entry"]:
        bad = [(C.c_void_p * 1)(None)] + args[1:] if k == "entry" else args[:k] + [None] + args[k + 1:]
        rc, msg = _raw(lib, who, *bad)
        assert rc != 0 and f"{who}: null argument" in msg, (k, msg)
    for n_a in (0, 65):
        rc, msg = _raw(lib, who, (C.c_void_p * 65)(*[plain.h] * 65), n_a, *args[2:])
        assert rc != 0 and who in msg and "between 1 and 64" in msg, msg
    assert plain.kernel_launches == n0
    # `a` fails the completeness rule
    A = Sharded(Engine, mol, 2, 1, par=SMALL)
    B = Sharded(Engine, mol, 2, 2, par=SMALL)
    for shards in ([A.eng[0]], [A.eng[1], A.eng[0]], [A.eng[0], A.eng[1], plain]):
        _refused(lambda: call(snap, shards), who, A.eng + [plain], "ranks 0 .. P - 1 of one run")
    _refused(lambda: call(snap, [A.eng[0], B.eng[1]]), who, A.eng + B.eng, "different runs")
    # Hubbard-Holstein, no molecule, no vector on the enumerating side
    hh_run = golden_io.manifest()["hh_runs"]["hh_l6_m2000"]
    hh = Engine(None)
    hh.setup_hh(vec_nonz=100, max_dets=1000, **{k: hh_run[k] for k in ("n_elec", "n_sites", "eps", "U", "omega", "g", "gs_energy", "target_norm", "initiator", "seed")})
    _refused(lambda: call(snap, [hh]), who, [hh], "Hubbard-Holstein")
    hh.close()
    empty, bare = Engine(None), Engine(mol)
    _refused(lambda: call(snap, [empty]), who, [empty], "fries_set_molecule")
    _refused(lambda: call(snap, [bare]), who, [bare], "solution vector")
    empty.close()
    bare.close()
    # another molecule than the snapshot's: another shape; the same shape with other irreps
    other = Engine(mols("H2O"))
    other.setup(**SMALL)
    relabelled = Engine(dataclasses.replace(mol, irreps=np.zeros_like(mol.irreps)))
    relabelled.setup(**SMALL)
    with Snapshot([other]) as so, Snapshot([relabelled]) as sr:
        _refused(lambda: call(snap, [other]), who, [other], "different molecules")
        _refused(lambda: call(so, [plain]), who, [plain], "different molecules")
        _refused(lambda: call(so, A.eng), who, A.eng, "different molecules")
        _refused(lambda: call(snap, [relabelled]), who, [relabelled], "irreps")
        _refused(lambda: call(sr, [plain]), who, [plain], "irreps")
    other.close()
    relabelled.close()
    # hf_en and spin_parity: compared by fries_h_dot_ranks; the density matrices ignore hf_en and refuse any spin_parity != 0
    shifted, flipped = Engine(fcidump.synthetic("Ne", seed=777)), Engine(mol)
    shifted.setup(**SMALL)
    flipped.setup(**SMALL)
    flipped.set_spin_parity(1)
    with Snapshot([shifted]) as ss, Snapshot([flipped]) as sf:
        assert sf.info.n_entries == 1
        if kind == "h_dot":
            _refused(lambda: call(snap, [shifted]), who, [shifted], "hf_en")
            _refused(lambda: call(ss, [plain]), who, [plain], "hf_en")
            assert call(sf, [flipped]).n_src == 1          # equal parities are served
        else:
            assert same_bits(call(ss, [plain]), call(snap, [plain]))       # (both hold 100 x the Hartree-Fock determinant)
            _refused(lambda: call(sf, [flipped]), who, [flipped], "spin_parity")
        _refused(lambda: call(snap, [flipped]), who, [flipped], "spin_parity")
        _refused(lambda: call(sf, [plain]), who, [plain], "spin_parity")
        flipped.set_spin_parity(0)
        A.eng[0].set_spin_parity(-1)
        _refused(lambda: call(snap, A.eng), who, A.eng, "spin_parity")
        A.eng[0].set_spin_parity(0)
    # the two-context entry points keep refusing a communicator (pair_common.check_common_refusals pins that); the served case
    with Snapshot(A.eng) as sa:
        assert call(sa, A.eng).n_src == 1 and call(snap, A.eng).n_src == 1
    snap.close()
    for x in (A, B, shifted, flipped, plain):
        x.close()


# ------------------------------------------------------------------ 6. reads only
def test_snapshot_and_estimators_do_not_disturb_a_sharded_run(Engine, Snapshot, mols):
    mol = mols("Ne")
    quiet, probed = Sharded(Engine, mol, 2, 1), Sharded(Engine, mol, 2, 1)
    quiet.iterate(20)
    probed.iterate(10)
    with Snapshot(probed.eng) as sn:
        got = _all_three(sn, probed.eng)
        assert got[0].n_hits > 0 and got[1].n_src == got[0].n_src and got[2].n_hits > 0
    probed.iterate(10)
    assert quiet.log_bytes() == probed.log_bytes()
    for k, ((dq, vq), (dp, vp)) in enumerate(zip(quiet.vectors(), probed.vectors())):
        assert dq.tobytes() == dp.tobytes() and vq.tobytes() == vp.tobytes(), k
    quiet.close()
    probed.close()


# ------------------------------------------------------------------ 7. memory
def test_snapshots_return_their_device_memory(Engine, Snapshot, mols):
    def call(a, b):
        with Snapshot([b]) as sn:
            assert sn.info.device_bytes > 0
            r = _all_three(sn, [a])
        assert r[1].n_src == r[0].n_src == r[2].n_src
        return r[0]

    pc.check_device_memory_returned(Engine, mols("Ne"), call, "fries_snapshot_create + the three estimators over ranks")


# ------------------------------------------------------------------ 8. FriReplicas
def test_sharded_replicas(Engine, Snapshot, mols):
    from fries_amd.replicas import FriReplicas
    mol = mols("Ne")
    par = pc.ne_run()
    seed = par.pop("seed")
    reps = FriReplicas(mol, 2, seed, ranks=2, **par)
    logs = reps.iterate(20)
    assert len(reps.shards) == 2 and all(len(sh) == 2 for sh in reps.shards) and len(reps.engines) == 4 and len(logs) == 2
    for r in range(2):
        lone = Sharded(Engine, mol, 2, seed + r, par=par, n_iter=20)
        for k in range(2):
            assert logs[r][k].tobytes() == lone.log_bytes()[k], (r, k)
            (dl, vl), (dr, vr) = lone.eng[k].vector(), reps.shards[r][k].vector()
            assert dl.tobytes() == dr.tobytes() and vl.tobytes() == vr.tobytes(), (r, k)
        lone.close()
    assert logs[0][0].tobytes() != logs[1][0].tobytes()
    sizes = [sum(e.vec_info()[1] for e in sh) for sh in reps.shards]
    a, b = (0, 1) if sizes[0] <= sizes[1] else (1, 0)
    est, g1, g2 = reps.pair_estimates(), reps.pair_rdm1(), reps.pair_rdm2()
    all_est, all_g1, all_g2 = reps.pair_all()           # one set of snapshots for the three: the same bits
    assert all_est == est and same_bits(all_g1[0], g1[0]) and same_bits(all_g2[0], g2[0])
    assert reps.pairs() == [(0, 1)] and len(est) == len(g1) == len(g2) == 1
    with Snapshot(reps.shards[b]) as sn:
        hd, r1, r2 = _all_three(sn, reps.shards[a])
    if a == 1:
        r1, r2 = r1.transposed(), r2.transposed()
    assert est[0] == hd and est[0].n_hits > 0 and same_bits(g1[0], r1) and same_bits(g2[0], r2)
    reps.close()
    assert reps.engines == [] and reps.shards == []
    # ranks == 1: the calls of the one-rank replicas, bit for bit
    ones = FriReplicas(mol, 2, seed, **par)
    ones.iterate(20)
    nz = [e.vec_info()[1] for e in ones.engines]
    a, b = (0, 1) if nz[0] <= nz[1] else (1, 0)
    ea, eb = ones.engines[a], ones.engines[b]
    assert ones.pair_estimates() == [ea.h_dot(eb)]
    want1, want2 = ea.rdm1(eb), ea.rdm2(eb)
    assert same_bits(ones.pair_rdm1()[0], want1 if a == 0 else want1.transposed())
    assert same_bits(ones.pair_rdm2()[0], want2 if a == 0 else want2.transposed())
    all_est, all_g1, all_g2 = ones.pair_all()
    assert all_est == [ea.h_dot(eb)] and same_bits(all_g1[0], ones.pair_rdm1()[0]) and same_bits(all_g2[0], ones.pair_rdm2()[0])
    ones.close()
