"""Device memory goes back to the device (-m gpu): a context returns everything it allocated on fries_ctx_destroy, the entry points
that work on temporaries return them when they leave, and a call that fails leaves the engine as it was.

How the bounds below were measured, and the figures, are in DESIGN.md ("Memory ownership")."""
import ctypes as C

import numpy as np
import pytest

import golden_io

pytestmark = pytest.mark.gpu

MIB = 1 << 20
N_CYCLES = 8
# the smallest parameters the suite uses for the Ne-shaped molecule
NE = dict(epsilon=0.01, vec_nonz=100, mat_nonz=100, max_dets=1000)
# Free memory the 8 cycles may cost, per driver kind.  At least twice the noise: 8 cycles of create + close alone cost 0 bytes in 36 of
# 40 readings and 2, 2, 6 and 8 MiB in the others (the runtime hands memory out in 2 MiB blocks, and the reading is device-wide).  At most
# half of what the code lost before the contexts owned their memory: 1420 MiB (frisys), 690 (full), 694 (fciqmc), 696 (multi), 1392 (hh).
# DESIGN.md section 4a has the measurements.
TOLERANCE = {kind: 32 * MIB for kind in ("frisys", "full", "fciqmc", "multi", "hh")}


def _free_bytes():
    """The device's free memory, device-wide: hipMemGetInfo of the HIP runtime the engine runs on, reached through the engine's library.
    (torch.cuda.mem_get_info reads the same counter, but torch ships a HIP runtime of its own, and that cannot initialise in a process
    in which the engine's already has -- which is every process that ran an engine test before this one.)"""
    from fries_amd.engine import load_library
    lib = load_library()
    free, total = C.c_size_t(), C.c_size_t()
    assert lib.hipDeviceSynchronize() == 0 and lib.hipMemGetInfo(C.byref(free), C.byref(total)) == 0
    return free.value


def _cycle(kind, mol):
    """create, set up, iterate 3 times, the entry points that work on temporaries once each, close"""
    from fries_amd.engine import FriEngine
    eng = FriEngine(None if kind == "hh" else mol)
    if kind == "frisys":
        # a dense space (the Hartree-Fock determinant), so that the dense block of H is tabulated.  Its 984 symmetry-allowed excitations
        # come off the matrix sample budget, which the setup requires to stay positive: mat_nonz = 100 cannot hold a dense space of
        # this molecule, 1100 is the next round figure that can; and the vector has to hold the 984 exact products beside the 1100 spawns.
        par = dict(NE, mat_nonz=1100, max_dets=4000)
        eng.setup(seed=1, det_space=np.array([_hf_det(mol)], dtype=np.uint64), **par)
        eng.iterate(3)
        for n_samp in (100, 600, 1100):     # PivBuf and FlatPiv are allocated, then outgrown
            eng.apply_hbpp_piv(n_samp)
        eng.compress_vec_piv(50)
    elif kind == "full":
        # (H applied in full to 100 determinants reaches some 1e5 of them: the vector and the spawn list have to hold those)
        eng.setup_full(epsilon=NE["epsilon"], vec_nonz=NE["vec_nonz"], max_dets=200000, seed=1, spawn_cap=300000)
        eng.iterate_full(3)
    elif kind == "fciqmc":
        eng.setup_fciqmc(epsilon=NE["epsilon"], target_walkers=100, max_dets=NE["max_dets"], seed=1)
        eng.iterate_fciqmc(3)
    elif kind == "multi":
        eng.setup_multi(seed=1, **NE)
        eng.iterate_multi(3)
    else:
        r = golden_io.manifest()["hh_runs"]["hh_l6_m2000"]      # the smallest lattice of the Hubbard-Holstein tests
        eng.setup_hh(n_elec=r["n_elec"], n_sites=r["n_sites"], eps=r["eps"], U=r["U"], omega=r["omega"], g=r["g"], gs_energy=r["gs_energy"],
                     vec_nonz=100, max_dets=1000, target_norm=r["target_norm"], initiator=r["initiator"], seed=r["seed"])
        eng.iterate_hh(3)
    if kind != "hh":        # (both need the molecule's integrals)
        hf = np.array([_hf_det(mol)], dtype=np.uint64)
        eng.matrel(0, hf)
        eng.h_offdiag_list(hf, np.ones(1))
    eng.test_teeth(0.25, 1.0, 100, np.linspace(0.0, 50.0, 7))
    eng.test_seqsum(np.linspace(-1.0, 1.0, 3000))
    eng.close()


def _hf_det(mol):
    half = (1 << (mol.n_elec // 2)) - 1
    return half | (half << mol.n_orb)


def _bare_cycle(kind, mol):
    from fries_amd.engine import FriEngine
    FriEngine(None if kind == "hh" else mol).close()


def lost_bytes(kind, mol, cycle=_cycle):
    """free device memory before minus after N_CYCLES cycles, one warm-up cycle first (code objects, the runtime's own pools)"""
    cycle(kind, mol)
    before = _free_bytes()
    for _ in range(N_CYCLES):
        cycle(kind, mol)
    return before - _free_bytes()


@pytest.mark.parametrize("kind", ["frisys", "full", "fciqmc", "multi", "hh"])
def test_contexts_return_their_device_memory(mols, kind):
    """Eight create / set up / iterate / close cycles of every driver kind cost no device memory.  The reading is device-wide, so
    another process's allocations show in it."""
    lost = lost_bytes(kind, mols("Ne"))
    print(f"{kind}: {lost} bytes ({lost / MIB:.1f} MiB) of free device memory lost over {N_CYCLES} cycles; bound {TOLERANCE[kind] / MIB:.0f} MiB")
    assert lost <= TOLERANCE[kind], (kind, lost)


def test_a_failed_call_leaves_the_engine_usable(mols):
    """A call that is refused after it has worked on temporaries raises, and the engine goes on as if the call had not been made.
    fries_h_offdiag_list with output buffers too small for the result is refused after fr_h_apply_list has built its temporary vector
    and spawn buffers in place of the context's and put the context's back.  (The host-side checks that sit between an allocation
    and its release all guard device errors, which a test does not provoke: this covers the error return and the state left behind,
    and vec_dot_list's up-front column check beside it.)"""
    from fries_amd.engine import FriEngine
    mol = mols("Ne")
    par = dict(NE, seed=1)
    ref = FriEngine(mol)
    ref.setup(**par)
    want = ref.iterate(5)
    ref.close()
    eng = FriEngine(mol)
    eng.setup(**par)
    first = eng.iterate(2)
    hf = np.array([_hf_det(mol)], dtype=np.uint64)
    one = np.ones(1)
    od, ov, m = np.zeros(1, dtype=np.uint64), np.zeros(1), C.c_size_t()
    with pytest.raises(RuntimeError, match="output buffers too small"):
        eng._ck(eng.lib.fries_h_offdiag_list(eng.h, hf.ctypes.data_as(C.c_void_p), one.ctypes.data_as(C.c_void_p), C.c_size_t(1),
                                             od.ctypes.data_as(C.c_void_p), ov.ctypes.data_as(C.c_void_p), C.c_size_t(1), C.byref(m)))
    out = C.c_double()
    with pytest.raises(RuntimeError, match="column must be 0 or 1"):
        eng._ck(eng.lib.fries_vec_dot_list(eng.h, 2, hf.ctypes.data_as(C.c_void_p), one.ctypes.data_as(C.c_void_p), C.c_size_t(1), C.byref(out)))
    assert eng.vec_info()[0] > 0
    got = np.concatenate([first, eng.iterate(3)])
    for f in want.dtype.names:
        assert np.array_equal(got[f], want[f]), f
    eng.close()
