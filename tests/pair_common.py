"""What the -m gpu tests of the estimators between two engines' vectors share (test_gpu_hdot.py, test_gpu_rdm1.py, test_gpu_rdm2.py):
the small helpers, the vectors several of them start from, and the three bodies that are the same for every estimator -- the refusals of
the common frame (csrc/pair_frame.hpp), "the estimator does not disturb the run" and "the estimator returns its device memory".
`call(a, b)` is the estimator under test as a function of two engines, `who` the name of its entry point."""
import ctypes as C
import dataclasses
import os
import subprocess

import numpy as np
import pytest

import golden_io

U = 2.0 ** -53
SMALL = dict(epsilon=0.01, vec_nonz=100, mat_nonz=100, max_dets=1000, seed=1, distribution="HB_unnorm")
NE_PAIR = dict(epsilon=0.01, vec_nonz=150, mat_nonz=150, max_dets=4000, target_norm=100.0, distribution="HB_unnorm")


def ne_run():
    r = golden_io.manifest()["runs"]["ne_m2000_unnorm"]
    return dict(epsilon=r["epsilon"], vec_nonz=r["vec_nonz"], mat_nonz=r["mat_nonz"], max_dets=r["max_dets"], target_norm=r["target_norm"],
                initiator=r["initiator"], seed=r["seed"], distribution=r["distribution"])


def as_map(dets, vals):
    return {int(d): float(v) for d, v in zip(dets, vals) if v != 0.0}


def same_bits(x, y):
    """two Rdm1 or two Rdm2: the array, then the scalars"""
    return np.array_equal(x[0], y[0]) and x[1:] == y[1:]


# ------------------------------------------------------------------ vectors
def min4_pair(Engine, mol, seed):
    """2 electrons in 4 orbitals, C1: all 16 determinants in both vectors, in different orders, two exact zeros each.
    -> the two engines, the determinants and what was loaded"""
    dets = np.array([(1 << p) | (1 << (mol.n_orb + q)) for p in range(4) for q in range(4)], dtype=np.uint64)
    rng = np.random.RandomState(seed)
    ea, eb = Engine(mol), Engine(mol)
    for e in (ea, eb):
        e.setup(epsilon=0.01, vec_nonz=50, mat_nonz=50, max_dets=1000, seed=3, distribution="HB_unnorm")
    da, db = dets[rng.permutation(16)], dets[rng.permutation(16)]
    va, vb = rng.standard_normal(16), rng.standard_normal(16)
    va[[3, 11]] = 0.0
    vb[[0, 7]] = 0.0
    ea.vec_load(da, va)
    eb.vec_load(db, vb)
    return ea, eb, dets, (da, va), (db, vb)


def ne_pair(Engine, mol):
    """Two Ne runs (seeds 1 and 2), 25 iterations at vec_nonz = mat_nonz = 150: compressed vectors with released positions and a hash
    table that has seen deletions"""
    ea, eb = Engine(mol), Engine(mol)
    ea.setup(seed=1, **NE_PAIR)
    eb.setup(seed=2, **NE_PAIR)
    ea.iterate(25)
    eb.iterate(25)
    return ea, eb


# ------------------------------------------------------------------ refusals
def refused(call, who, a, b, match):
    na, nb = a.kernel_launches, b.kernel_launches
    with pytest.raises(RuntimeError, match=match) as ex:
        call(a, b)
    assert who in str(ex.value)
    assert (a.kernel_launches, b.kernel_launches) == (na, nb)


def check_common_refusals(Engine, mols, plain, call, who, result, out=None):
    """What every estimator refuses before it launches anything.  plain: an engine with a molecule and a solution vector, which the
    other engines are made to differ from; result: the entry point's result struct; out: the array it fills besides, if it has one."""
    from fries_amd.comm import LocalGroup
    mol = plain.mol
    # null arguments
    args = [plain.h, plain.h] + ([out.ctypes.data_as(C.c_void_p)] if out is not None else []) + [C.byref(result())]
    n0 = plain.kernel_launches
    for k in range(len(args)):
        assert getattr(plain.lib, who)(*(args[:k] + [None] + args[k + 1:])) != 0
        assert f"{who}: null argument" in plain.lib.fries_last_error().decode()
    assert plain.kernel_launches == n0
    # a communicator, even of one rank
    grp = LocalGroup(1, SMALL["mat_nonz"])
    ranked = Engine(mol, comm=grp.comm(0, 0))
    ranked.setup(**SMALL)
    refused(call, who, plain, ranked, "communicator")
    refused(call, who, ranked, plain, "communicator")
    refused(call, who, ranked, ranked, "communicator")
    ranked.close()
    grp.destroy()
    # Hubbard-Holstein
    hh_run = golden_io.manifest()["hh_runs"]["hh_l6_m2000"]
    hh = Engine(None)
    hh.setup_hh(vec_nonz=100, max_dets=1000, **{k: hh_run[k] for k in ("n_elec", "n_sites", "eps", "U", "omega", "g", "gs_energy", "target_norm", "initiator", "seed")})
    refused(call, who, hh, hh, "Hubbard-Holstein")
    refused(call, who, plain, hh, "Hubbard-Holstein")
    hh.close()
    # no molecule; no solution vector yet
    empty = Engine(None)
    refused(call, who, plain, empty, "fries_set_molecule")
    empty.close()
    bare = Engine(mol)
    refused(call, who, plain, bare, "solution vector")
    refused(call, who, bare, plain, "solution vector")
    bare.close()
    # different molecules: another shape; the same shape with other irreps
    assert (mol.n_orb, mol.n_elec) != (mols("H2O").n_orb, mols("H2O").n_elec) and np.any(np.asarray(mol.irreps) != 0)
    other = Engine(mols("H2O"))
    other.setup(**SMALL)
    refused(call, who, plain, other, "different molecules")
    refused(call, who, other, plain, "different molecules")
    other.close()
    relabelled = Engine(dataclasses.replace(mol, irreps=np.zeros_like(mol.irreps)))
    relabelled.setup(**SMALL)
    refused(call, who, plain, relabelled, "irreps")
    relabelled.close()


def check_density_matrix_refusals(Engine, plain, call, who):
    """... and what fries_rdm1 and fries_rdm2 add (fr_pair_begin_rdm) or, unlike fries_h_dot, leave out"""
    from fries_amd import fcidump
    # the same shape with other integrals is NOT refused: hf_en plays no part
    shifted = Engine(fcidump.synthetic("Ne", seed=777))
    shifted.setup(**SMALL)
    assert shifted.hf_energy != plain.hf_energy
    assert same_bits(call(plain, shifted), call(plain, plain))      # (both hold 100 x the Hartree-Fock determinant)
    shifted.close()
    # time-reversal vectors, on either side
    flipped = Engine(plain.mol)
    flipped.setup(**SMALL)
    for sp in (1, -1):
        flipped.set_spin_parity(sp)
        refused(call, who, plain, flipped, "spin_parity")
        refused(call, who, flipped, plain, "spin_parity")
        refused(call, who, flipped, flipped, "spin_parity")
    flipped.set_spin_parity(0)
    assert same_bits(call(plain, flipped), call(plain, plain))
    flipped.close()


# ------------------------------------------------------------------ the estimator reads, and only reads
def assert_same_run(quiet, probed, log_quiet, log_probed, tag=None):
    assert log_quiet.tobytes() == log_probed.tobytes(), tag
    (dq, vq), (dp, vp) = quiet.vector(), probed.vector()
    assert dq.tobytes() == dp.tobytes() and vq.tobytes() == vp.tobytes(), tag       # (every byte: more than a digest)


def check_run_undisturbed(Engine, mol, call):
    """Two runs of 20 iterations with the estimator called between them half-way, every way round, against two that are left alone"""
    par = ne_run()
    quiet_a, quiet_b, probed_a, probed_b = (Engine(mol) for _ in range(4))
    for e, seed in ((quiet_a, par["seed"]), (quiet_b, par["seed"] + 1), (probed_a, par["seed"]), (probed_b, par["seed"] + 1)):
        e.setup(**dict(par, seed=seed))
    want = [quiet_a.iterate(20), quiet_b.iterate(20)]
    first = [probed_a.iterate(10), probed_b.iterate(10)]
    res = call(probed_a, probed_b)
    assert res.n_hits > 0 and call(probed_b, probed_a).n_hits == res.n_hits and call(probed_a, probed_a).n_src > 0
    got = [np.concatenate([first[0], probed_a.iterate(10)]), np.concatenate([first[1], probed_b.iterate(10)])]
    for k, (q, p) in enumerate(((quiet_a, probed_a), (quiet_b, probed_b))):
        assert_same_run(q, p, want[k], got[k], k)
    for e in (quiet_a, quiet_b, probed_a, probed_b):
        e.close()


# ------------------------------------------------------------------ device memory
def check_device_memory_returned(Engine, mol, call, who):
    """The estimator's scratch comes from a stack DevMem: added to the create / set up / iterate / close cycle of tests/test_gpu_memory.py,
    that test's bound keeps holding."""
    import test_gpu_memory as tm

    def cycle(kind, mol):
        a, b = Engine(mol), Engine(mol)
        a.setup(seed=1, **tm.NE)
        b.setup(seed=2, **tm.NE)
        a.iterate(3)
        b.iterate(3)
        assert call(a, b).n_src > 0 and call(b, b).n_src > 0
        a.close()
        b.close()

    lost = tm.lost_bytes("frisys", mol, cycle)
    print(f"{lost} bytes of free device memory lost over {tm.N_CYCLES} cycles with {who}; bound {tm.TOLERANCE['frisys']}")
    assert lost <= tm.TOLERANCE["frisys"]


# ------------------------------------------------------------------ the command line
def cmd(exe, fc, mol, par, n_it, out, seed):
    return [exe, "--fcidump_path", fc, "--point_group", mol.point_group, "--distribution", par["distribution"], "--vec_nonz", str(par["vec_nonz"]),
            "--mat_nonz", str(par["mat_nonz"]), "--max_dets", str(par["max_dets"]), "--target", repr(par["target_norm"]), "--initiator", repr(par["initiator"]),
            "--epsilon", repr(par["epsilon"]), "--max_iter", str(n_it), "--result_dir", out, "--seed", str(seed), "--precision", "17"]


def saved_vector(out, mol):
    nb = (2 * mol.n_orb + 7) // 8
    raw = np.fromfile(out + "dets0.dat", dtype=np.uint8)
    n_saved = raw.size // nb
    vals = np.fromfile(out + "vals0.dat", dtype=np.float64)
    dets = np.zeros(n_saved, dtype=np.uint64)
    for b in range(nb):
        dets |= raw.reshape(n_saved, nb)[:, b].astype(np.uint64) << np.uint64(8 * b)
    vals = vals[:n_saved]
    return dets[vals != 0], vals[vals != 0]


def run(cmd_line):
    res = subprocess.run(cmd_line, capture_output=True, text=True, timeout=300)
    assert res.returncode == 0 and "Exception" not in res.stderr, res.stderr[-3000:]


def tree(top):
    out = {}
    for dp, _, fs in os.walk(top):
        for f in fs:
            p = os.path.join(dp, f)
            with open(p, "rb") as fh:
                out[os.path.relpath(p, top)] = fh.read()
    return out
