"""Vector snapshots and the estimators over ranks as a boundary, checked without a GPU: libfries_hip.so exports the seven entry points,
include/fries_hip.h declares them and the info struct, the Python layer lists and wraps them, FriReplicas takes `ranks`, and the sizing
of csrc/snapshot_plan.hpp passes a stand-alone replay under AddressSanitizer and UBSan."""
import ctypes
import inspect
import os
import re
import subprocess

from fries_amd import engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("fries_snapshot_create", "fries_snapshot_info", "fries_snapshot_vector", "fries_snapshot_destroy",
                "fries_h_dot_ranks", "fries_rdm1_ranks", "fries_rdm2_ranks")


def test_library_exports_the_seven_entry_points():
    assert os.path.exists(engine.LIB_PATH), "libfries_hip.so has not been built"
    lib = ctypes.CDLL(engine.LIB_PATH)
    for name in ENTRY_POINTS:
        assert hasattr(lib, name), name


def test_header_declares_them_and_the_info_struct():
    with open(os.path.join(ROOT, "include", "fries_hip.h")) as f:
        header = f.read()
    sp = r"\s*"
    shards = r"fries_ctx\s*\*\s*const\s*\*\s*"
    snap = r"const\s+fries_snapshot\s*\*\s*"
    cm = r"(/\*.*?\*/)?\s*"
    decls = {
        "fries_snapshot_create": r"fries_snapshot\s*\*\*\s*s\s*,\s*" + shards + r"shards\s*,\s*uint32_t\s+n_shards\s*,\s*int\s+device",
        "fries_snapshot_info": snap + r"s\s*,\s*fries_snapshot_info_t\s*\*\s*out",
        "fries_snapshot_vector": snap + r"s\s*,\s*uint64_t\s*\*\s*dets\s*,\s*double\s*\*\s*vals\s*,\s*uint64_t\s+cap\s*,\s*uint64_t\s*\*\s*n",
        "fries_snapshot_destroy": r"fries_snapshot\s*\*\s*s",
        "fries_h_dot_ranks": shards + r"a\s*,\s*uint32_t\s+n_a\s*,\s*" + snap + r"b\s*,\s*fries_hdot_result\s*\*\s*out",
        "fries_rdm1_ranks": shards + r"a\s*,\s*uint32_t\s+n_a\s*,\s*" + snap + r"b\s*,\s*double\s*\*\s*gamma\s*" + cm + r",\s*fries_rdm1_result\s*\*\s*out",
        "fries_rdm2_ranks": shards + r"a\s*,\s*uint32_t\s+n_a\s*,\s*" + snap + r"b\s*,\s*double\s*\*\s*gamma2\s*" + cm + r",\s*fries_rdm2_result\s*\*\s*out",
    }
    assert set(decls) == set(ENTRY_POINTS)
    for name, args in decls.items():
        assert re.search(r"\bint\s+" + name + sp + r"\(" + sp + args + sp + r"\)" + sp + ";", header), name
    assert re.search(r"typedef\s+struct\s+fries_snapshot\s+fries_snapshot\s*;", header)
    m = re.search(r"typedef\s+struct\s*\{([^}]*)\}\s*fries_snapshot_info_t\s*;", header)
    assert m, "struct fries_snapshot_info_t is not declared"
    body = " ".join(m.group(1).split())
    assert body == "uint64_t n_entries; uint32_t n_shards, n_slots; uint64_t device_bytes; int32_t device; float ms_compact, ms_copy, ms_insert;", body
    # the comment states how a snapshot is built, the completeness rule, the threading contract, determinism and what is out of scope
    flat = " ".join(header.replace("\n *", " ").split())       # (a phrase may run over a line break of the comment)
    for phrase in ("hipMemcpyPeerAsync", "rank order", "position order", "40 %", "ranks 0 .. n_shards - 1 of one run, in order", "may be inside another call",
                   "in rank order", "bit for bit", "before the first launch", "an empty shard launches nothing", "separate processes", "more than one GPU"):
        assert phrase in flat, phrase


def test_python_layer_lists_and_wraps_them():
    for name in ENTRY_POINTS:
        assert name in engine.EXPORTS, name
    assert ctypes.sizeof(engine.SnapshotInfoStruct) == 40
    assert [f[0] for f in engine.SnapshotInfoStruct._fields_] == ["n_entries", "n_shards", "n_slots", "device_bytes", "device", "ms_compact", "ms_copy", "ms_insert"]
    assert engine.SnapshotInfo._fields == ("n_entries", "n_shards", "n_slots", "device_bytes", "device", "ms_compact", "ms_copy", "ms_insert")
    snap = engine.VecSnapshot
    assert list(inspect.signature(snap.__init__).parameters)[1:] == ["shards", "device"]
    assert inspect.signature(snap.__init__).parameters["device"].default is None
    for meth in ("vector", "close", "h_dot", "rdm1", "rdm2", "__enter__", "__exit__"):
        assert callable(getattr(snap, meth, None)), meth
    assert isinstance(snap.info, property)


def test_replicas_take_ranks():
    from fries_amd.replicas import FriReplicas
    par = inspect.signature(FriReplicas.__init__).parameters
    assert par["ranks"].default == 1 and par["devices"].default is None
    assert list(par)[:4] == ["self", "mol", "n", "seed"]
    assert par["device"].default == 0           # (where the one-rank replicas have always taken their device)
    assert callable(getattr(FriReplicas, "pair_all", None))
    import pytest
    with pytest.raises(TypeError, match="mat_nonz"):        # (refused before an engine is created: no GPU needed)
        FriReplicas(None, 1, 0, ranks=2, epsilon=0.01, vec_nonz=10, max_dets=100)


def test_plan_replay_under_sanitizers(tmp_path):
    """tests/cpp/snapshot_plan_check.cpp, host only: g++ -fsanitize=address,undefined, its own main, nothing loaded into Python (the
    sanitizers' runtimes are linked statically, so that the program starts whatever else the loader brings in).  Its cases include one
    entry, an empty shard between full ones and counts on either side of a slot-count doubling."""
    exe = str(tmp_path / "snapshot_plan_check")
    src = os.path.join(ROOT, "tests", "cpp", "snapshot_plan_check.cpp")
    res = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-o", exe, src], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr[-3000:]
    res = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(res.stdout[-2000:])
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-3000:]
    assert re.search(r"\b\d+ geometries, 0 failures\b", res.stdout)
