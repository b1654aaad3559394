"""-m gpu: one FRI iteration of frisys_mol step by step (fries_apply_hbpp_sys without download, fries_spawn_from_comp, fries_dense_apply,
fries_death_clone, fries_dots, fries_find_preserve, fries_dense_norm, fries_sys_comp) must be the fused iteration: against the reference's
golden trajectories, against fries_frisys_iterate call by call, over ranks, and through include/FRIES/device_loop.hpp from a C++ loop
that keeps the reference's shape.  Every comparison is equality (with ranks: numerator / denominator as tests/ranks_worker.py compares them)."""
import ctypes as C
import json
import os
import re
import socket
import subprocess
import sys

import numpy as np
import pytest

import golden_io
from fries_amd import fcidump

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# RUNS[0] of test_gpu_parity.py
NE = dict(epsilon=0.01, vec_nonz=2000, mat_nonz=2000, max_dets=20000, target_norm=1000.0, initiator=1.0, seed=20250215, distribution="HB_unnorm")
# kernel launches of the fused engine over setup + 30 x (iterate(1), vector()) of the NE run, as counted on the commit before the stepwise
# entry points existed: the fused loop must enqueue exactly what it enqueued then
PARENT_FUSED_LAUNCHES = 10227


@pytest.fixture(scope="module")
def Engine():
    from fries_amd.engine import FriEngine
    return FriEngine


def _setup(Engine, mols, r, **kw):
    eng = Engine(mols(r["shape"]))
    eng.setup(epsilon=r["epsilon"], vec_nonz=r["vec_nonz"], mat_nonz=r["mat_nonz"], max_dets=r["max_dets"], target_norm=r["target_norm"],
              initiator=r["initiator"], seed=r["seed"], distribution=r["distribution"], **kw)
    return eng


def _check_rows(eng, rows, last=None):
    for row in rows:
        lg = eng.iterate_stepwise(1)[0]
        for f in ("nkept", "n_nonz", "curr_size", "num_success"):
            assert int(lg[f]) == row[f], (row["it"], f, int(lg[f]), row[f])
        for f in ("norm", "shift", "numer", "denom"):
            assert float(lg[f]) == row[f], (row["it"], f, float(lg[f]).hex(), row[f].hex())
        if row["it"] % 10 == 9 or row is last:
            d, v = eng.vector()
            assert golden_io.vec_hash(d, v) == row["hash"], row["it"]


@pytest.mark.parametrize("name", ["min4_m50_unnorm", "ne_m2000_unnorm", "h2o_m5000_hb", "n2_m10000_unnorm_ini0"])
def test_stepwise_trajectory_matches_reference_golden(Engine, mols, name):
    r = golden_io.manifest()["runs"][name]
    g = golden_io.read_traj(name)
    eng = _setup(Engine, mols, r)
    assert eng.p_doub == g["p_doub"] and eng.hf_energy == g["hf_en"]
    assert eng.dense_h_count() == 0 and eng.dense_norm() == 0.0
    _check_rows(eng, g["rows"], g["rows"][-1])
    eng.close()


@pytest.mark.parametrize("name", ["ne_m2000_dense", "n2_m10000_dense_hb"])
def test_stepwise_dense_space_matches_reference_golden(Engine, mols, name):
    """dense_apply, dense_norm and the budget mat_nonz - dense_h_count."""
    r = golden_io.manifest()["dense_runs"][name]
    g = golden_io.read_traj(name)
    space = np.array([int(x) for x in open(os.path.join(golden_io.GOLD, r["det_space"])).read().split()], dtype=np.uint64)
    eng = _setup(Engine, mols, r, det_space=space)
    assert 0 < eng.dense_h_count() < r["mat_nonz"]
    _check_rows(eng, g["rows"], g["rows"][-1])
    d, _ = eng.vector()
    assert np.array_equal(d[:space.size], space)
    eng.close()


def test_stepwise_equals_fused_call_by_call(Engine, mols):
    mol = mols("Ne")
    fused, step = Engine(mol), Engine(mol)
    fused.setup(**NE)
    step.setup(**NE)
    for it in range(30):
        lf, ls = fused.iterate(1)[0], step.iterate_stepwise(1)[0]
        for f in ("numer", "denom", "shift", "norm", "nkept", "n_nonz", "curr_size", "num_success"):
            assert lf[f] == ls[f], (it, f, lf[f], ls[f])
        assert lf["comp_len"].tolist() == ls["comp_len"].tolist(), it
        assert int(lf["err"]) == 0
        (df, vf), (ds, vs) = fused.vector(), step.vector()
        assert vf.tobytes() == vs.tobytes() and np.array_equal(df[vf != 0], ds[vs != 0]), it
    launches = fused.kernel_launches
    print("fused kernel launches:", launches, "stepwise:", step.kernel_launches)
    assert launches == PARENT_FUSED_LAUNCHES
    fused.close()
    step.close()


def _column(eng, col):
    n = eng.vec_info()[0]
    out = np.zeros(max(n, 1))
    m = C.c_size_t()
    eng._ck(eng.lib.fries_vec_column_download(eng.h, col, out.ctypes.data_as(C.c_void_p), out.size, C.byref(m)))
    return out[:m.value]


def test_pivotal_compression_feeds_spawn_from_comp(Engine, mols):
    """apply_hbpp_piv + spawn_from_comp on one engine against comp_download + host-built spawns + fries_vec_add_to(column 1) on another."""
    mol = mols("Ne")
    a, b = Engine(mol), Engine(mol)
    a.setup(**NE)
    b.setup(**NE)
    a.iterate(5)
    d, v = a.vector()
    d, v = d[v != 0], v[v != 0]
    a.vec_load(d, v)        # both engines hold the same vector in the same layout (no released positions)
    b.vec_load(d, v)
    a.restart(4242)
    pos, orbs, vals, _ = a.apply_hbpp_piv(2000)
    assert pos.size > 0
    pos2, orbs2, vals2 = a.comp_download()
    assert np.array_equal(pos, pos2) and np.array_equal(orbs, orbs2) and vals.tobytes() == vals2.tobytes()
    eps, thresh = NE["epsilon"], NE["initiator"]
    a.spawn_from_comp(eps, thresh)
    # frisys_mol.cpp:435-464 on the host
    new_d = np.zeros(pos.size, dtype=np.uint64)
    add = np.zeros(pos.size)
    ini = np.zeros(pos.size, dtype=np.uint8)
    for j in range(pos.size):
        cur, det = float(v[pos[j]]), int(d[pos[j]])
        o1, o2, u1, u2 = (int(x) for x in orbs[j])
        el = -eps * float(vals[j])
        if cur < 0:
            el *= -1
        if not (u1 == 0 and u2 == 0):
            det = (det & ~(1 << o1) & ~(1 << o2)) | (1 << u1) | (1 << u2)
        else:
            det = (det & ~(1 << o1)) | (1 << o2)
        new_d[j], add[j], ini[j] = det, el, abs(cur) >= thresh
    order = np.concatenate([np.nonzero(ini == 0)[0], np.nonzero(ini == 1)[0]])      # non-initiator origins first, then initiators
    b.vec_add_to(1, new_d[order], add[order], ini[order])
    assert a.vec_info()[0] == b.vec_info()[0]
    ca, cb = _column(a, 1), _column(b, 1)
    assert np.count_nonzero(ca) > 0 and ca.tobytes() == cb.tobytes()
    assert np.array_equal(_column(a, 0), _column(b, 0))
    (da, _), (db, _) = a.vector(), b.vector()
    assert np.array_equal(da[ca != 0], db[cb != 0])
    a.close()
    b.close()


def test_stale_result_guard(Engine, mols):
    """spawn_from_comp refuses -- with a message, before any launch -- when no compression result is pending; the engine goes on."""
    r = golden_io.manifest()["runs"]["ne_m2000_unnorm"]
    g = golden_io.read_traj("ne_m2000_unnorm")
    eng = _setup(Engine, mols, r)
    n0 = eng.kernel_launches
    with pytest.raises(RuntimeError, match="no compression result is pending"):     # before any compression
        eng.spawn_from_comp(r["epsilon"], r["initiator"])
    with pytest.raises(RuntimeError, match="no compression result is pending"):
        eng.comp_download()
    assert eng.kernel_launches == n0
    _check_rows(eng, g["rows"][:12])            # the run goes on as if nothing had happened
    eng.close()

    eng = _setup(Engine, mols, r)
    eng.iterate_stepwise(3)
    rn = [0.5, 0.25, 0.75, 0.125, 0.625]        # uniforms of the test's own: the engine's generator is left alone
    # twice in a row
    n_succ, _ = eng.apply_hbpp_sys_device(r["mat_nonz"], rn)
    assert n_succ > 0
    eng.spawn_from_comp(r["epsilon"], r["initiator"])
    n1 = eng.kernel_launches
    with pytest.raises(RuntimeError, match="no compression result is pending"):
        eng.spawn_from_comp(r["epsilon"], r["initiator"])
    assert eng.kernel_launches == n1
    eng.death_clone(r["epsilon"], 0.0, eng.vec_info()[0])       # column 1 back to zero
    # an intervening vec_load
    eng.apply_hbpp_sys_device(r["mat_nonz"], rn)
    d, v = eng.vector()
    eng.vec_load(d[v != 0], v[v != 0])
    n2 = eng.kernel_launches
    with pytest.raises(RuntimeError, match="no compression result is pending"):
        eng.spawn_from_comp(r["epsilon"], r["initiator"])
    assert eng.kernel_launches == n2
    # still usable: both loops run on
    assert int(eng.iterate(1)[0]["err"]) == 0
    lg = eng.iterate_stepwise(1)[0]
    assert int(lg["n_nonz"]) > 0 and float(lg["denom"]) != 0
    eng.close()


# ------------------------------------------------------------------ ranks
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _run_ranks(cmd, env, timeout):
    import signal
    proc = subprocess.Popen(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, start_new_session=True)
    try:
        out, err = proc.communicate(timeout=timeout)
    except subprocess.TimeoutExpired:
        os.killpg(proc.pid, signal.SIGKILL)
        out, err = proc.communicate()
        pytest.fail(f"ranks did not finish within {timeout} s\n" + out[-2000:] + err[-4000:])
    return subprocess.CompletedProcess(cmd, proc.returncode, out, err)


@pytest.mark.parametrize("name", ["n2_m10000_unnorm_p2", "ne_m2000_dense_p2", "n2_m10000_unnorm_p2_adder300"])
def test_stepwise_over_ranks_matches_reference_ranks(name, tmp_path):
    """iterate_stepwise on every rank (tests/stepwise_worker.py under torch.distributed.run, gloo, all ranks on one GPU) against what the
    same rank of the reference logged under mpiexec: spawn_from_comp as a collective, the dense block exchanged over ranks, and an Adder of
    300 elements (several perform_add rounds per pass)."""
    man = golden_io.manifest()
    r = next(man[k][name] for k in ("mpi_runs", "dense_mpi_runs", "adder_runs") if name in man.get(k, {}))
    P = r["n_ranks"]
    assert P <= 3
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", OMP_NUM_THREADS="1")
    if "adder_size" in r:
        env["FRIES_ADDER_SIZE"] = str(r["adder_size"])
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={P}", "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), os.path.join(ROOT, "tests", "stepwise_worker.py"), name, "gloo", str(tmp_path)]
    res = _run_ranks(cmd, env, 300)
    for k in range(P):
        fn = tmp_path / f"rank{k}.json"
        assert fn.exists(), res.stdout[-2000:] + res.stderr[-4000:]
        rep = json.loads(fn.read_text())
        assert rep["ok"], rep["fails"]
        assert rep["iters"] == r["n_iter"]
        if "adder_size" in r:
            assert rep["n_alltoallv"] > 2 * rep["iters"], rep        # the rounds did take place
        elif "det_space" not in r:
            assert rep["n_alltoallv"] == rep["iters"]               # one spawn exchange per iteration, as in the fused loop
    assert res.returncode == 0, res.stderr[-4000:]


# ------------------------------------------------------------------ the C++ consumer of include/FRIES/device_loop.hpp
def _cmd(exe, fc, mol, r, n_it, out):
    return [exe, "--fcidump_path", fc, "--point_group", mol.point_group, "--distribution", r["distribution"], "--vec_nonz", str(r["vec_nonz"]),
            "--mat_nonz", str(r["mat_nonz"]), "--max_dets", str(r["max_dets"]), "--target", repr(r["target_norm"]), "--initiator", repr(r["initiator"]),
            "--epsilon", repr(r["epsilon"]), "--max_iter", str(n_it), "--result_dir", out, "--seed", str(r["seed"])]


def _saved_vector(out, mol):
    nb = (2 * mol.n_orb + 7) // 8
    raw = np.fromfile(out + "dets0.dat", dtype=np.uint8)
    n_saved = raw.size // nb
    vals = np.fromfile(out + "vals0.dat", dtype=np.float64)
    assert vals.size == 2 * n_saved and np.all(vals[n_saved:] == 0)
    dets = np.zeros(n_saved, dtype=np.uint64)
    for b in range(nb):
        dets |= raw.reshape(n_saved, nb)[:, b].astype(np.uint64) << np.uint64(8 * b)
    return dets, vals[:n_saved]


@pytest.mark.parametrize("name", ["ne_m2000_unnorm", "n2_m30000_unnorm", "ne_m2000_dense"])
def test_device_loop_consumer_matches_reference(name, tmp_path):
    from fries_amd import build
    man = golden_io.manifest()
    r = man["runs"][name] if name in man["runs"] else man["dense_runs"][name]
    g = golden_io.read_traj(name)
    mol = fcidump.synthetic(r["shape"])
    fc = str(tmp_path / "mol.FCIDUMP")
    fcidump.write_fcidump(fc, mol)
    out = str(tmp_path / "run") + "/"
    os.makedirs(out)
    assert os.path.exists(build.DEVICE_LOOP_DRIVER), "frisys_mol_device_loop has not been built"
    n_it = min(r["n_iter"], 40)
    cmd = _cmd(build.DEVICE_LOOP_DRIVER, fc, mol, r, n_it, out)
    if "det_space" in r:
        cmd += ["--det_space", os.path.join(golden_io.GOLD, r["det_space"])]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert res.returncode == 0 and "Exception" not in res.stderr, res.stderr[-2000:]
    num = np.loadtxt(out + "projnum.txt"); den = np.loadtxt(out + "projden.txt"); nk = np.loadtxt(out + "nkept.txt")
    sh = np.loadtxt(out + "S.txt").reshape(-1); nm = np.loadtxt(out + "norm.txt").reshape(-1)
    assert num.size == n_it
    for i in range(n_it):
        row = g["rows"][i]
        assert int(nk[i]) == row["nkept"], i
        assert num[i] == row["numer"] and den[i] == row["denom"], (i, num[i], row["numer"], den[i], row["denom"])
    for k in range(n_it // 10):
        row = g["rows"][10 * k + 9]
        assert sh[k] == row["shift"] and nm[k] == row["norm"], k
    dets, vals = _saved_vector(out, mol)
    assert dets.size == g["rows"][n_it - 1]["curr_size"]
    assert golden_io.vec_hash(dets, vals) == g["rows"][n_it - 1]["hash"]
    if "det_space" in r:
        assert open(out + "dense.txt").read().strip().rstrip(",") == str(r["n_dense"])


def _facade_bytes(exe, fc, mol, r, n_it, tmp_path, tag):
    out = str(tmp_path / f"{tag}{n_it}") + "/"
    os.makedirs(out)
    res = subprocess.run(_cmd(exe, fc, mol, r, n_it, out), capture_output=True, text=True, timeout=300, env=dict(os.environ, FRIES_FACADE_STATS="1"))
    assert res.returncode == 0 and "Exception" not in res.stderr, res.stderr[-2000:]
    m = re.search(r"fries facade: (\d+) bytes host->device, (\d+) bytes device->host", res.stderr)
    assert m, res.stderr[-2000:]
    n_saved = os.path.getsize(out + "dets0.dat") // ((2 * mol.n_orb + 7) // 8)
    return int(m.group(1)), int(m.group(2)), n_saved


def test_device_loop_consumer_moves_no_bulk_data(Engine, mols, tmp_path):
    """Per iteration (the difference of a 40- and a 20-iteration run): nothing device -> host, and host -> device at most the two dot
    lists -- no column mirror, no compression result, no spawn list.  The unmodified frisys_mol_ref_api keeps its traffic.
    The set-up is the same in both runs and drops out of the difference; the closing DistVec::save() is not -- it fetches the determinants
    and both columns of a vector that has grown in between, 24 bytes per stored position -- so it is taken off each run's total first."""
    from fries_amd import build
    r = golden_io.manifest()["runs"]["ne_m2000_unnorm"]
    mol = mols(r["shape"])
    fc = str(tmp_path / "mol.FCIDUMP")
    fcidump.write_fcidump(fc, mol)
    eng = _setup(Engine, mols, r)
    n_htrial, n_trial = len(eng.htrial()[0]), 1         # the trial vector is the Hartree-Fock determinant
    eng.close()
    bound = 16 * (n_htrial + n_trial)
    up20, down20, n20 = _facade_bytes(build.DEVICE_LOOP_DRIVER, fc, mol, r, 20, tmp_path, "dev")
    up40, down40, n40 = _facade_bytes(build.DEVICE_LOOP_DRIVER, fc, mol, r, 40, tmp_path, "dev")
    down20, down40 = down20 - 24 * n20, down40 - 24 * n40
    print("device loop, bytes per iteration: up", (up40 - up20) / 20, "down", (down40 - down20) / 20, "bound up", bound)
    assert down40 - down20 == 0
    assert 0 < up40 - up20 <= 20 * bound
    rup20, rdown20, _ = _facade_bytes(build.REF_API_DRIVER, fc, mol, r, 20, tmp_path, "ref")
    rup40, rdown40, _ = _facade_bytes(build.REF_API_DRIVER, fc, mol, r, 40, tmp_path, "ref")
    print("ref api, bytes per iteration: up", (rup40 - rup20) / 20, "down", (rdown40 - rdown20) / 20, "totals", rup20, rdown20, rup40, rdown40)
    assert (rup20, rdown20, rup40, rdown40) == REF_API_TRAFFIC


# (host->device, device->host) totals of frisys_mol_ref_api on ne_m2000_unnorm after 20 and after 40 iterations, as counted before
# include/FRIES/device_loop.hpp existed: callers that do not opt in see the façade they saw
REF_API_TRAFFIC = (1900232, 937728, 4138496, 2191144)
