"""GPU tests of the consistent orientation of normals and of the winding of a mesh (csrc/orient.hip, csrc/mesh_ops.hip bs_mesh_orient_*,
csrc/union_parity.h, bodyslam_amd/pointcloud.py, bodyslam_amd/mesh.py) against the statement tests/_orient_ref.py: bit-equal -- the flips,
the bytes of the normals or the triangles, and the number of trees.  tests/test_orient_cpu.py asserts that the inputs exercise what is
claimed for them."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _orient_ref as O  # noqa: E402

pytestmark = pytest.mark.gpu
f32 = np.float32


@pytest.fixture(scope="module")
def PC():
    import bodyslam_amd.pointcloud as PC
    return PC


@pytest.fixture(scope="module")
def M():
    import bodyslam_amd.mesh as M
    return M


_REF = {}


def ref(name, fn, *args):
    """the statement's result, computed once per case and left unchanged"""
    if name not in _REF:
        _REF[name] = fn(*args)
    return _REF[name]


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def check_cloud(PC, name, pts, nrm, k, direction=(0.0, 0.0, 1.0), cell_size=None):
    want = ref((name, k), O.orient_normals, pts, nrm, k, direction)
    out, flipped = PC.orient_normals_consistent_tangent_plane(pts, nrm, k, direction=direction, cell_size=cell_size)
    assert out.is_cuda and out.dtype == torch.float32 and flipped.is_cuda and flipped.dtype == torch.bool
    out, flipped = out.cpu().numpy(), flipped.cpu().numpy()
    assert np.array_equal(flipped, want[1]), (name, k, int((flipped != want[1]).sum()))
    assert same_bits(out, want[0]), (name, k)
    assert PC.last_components == want[2], (name, k, PC.last_components, want[2])
    assert 1 <= PC.last_rounds <= len(pts) + 1
    return out, flipped


# ---- clouds ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cell_size", [None, 0.05])
def test_tube(PC, cell_size):
    pts, nrm = O.tube()
    start = O.random_signs(nrm, 5)
    out, _ = check_cloud(PC, "tube", pts, start, 10, cell_size=cell_size)
    assert same_bits(out, nrm) and PC.last_components == 1 and PC.last_rounds > 2


def test_tube_other_k_and_direction(PC):
    pts, nrm = O.tube()
    start = O.random_signs(nrm, 5)
    check_cloud(PC, "tube", pts, start, 6)
    out, _ = check_cloud(PC, "tube down", pts, start, 16, direction=(0.0, 0.0, -1.0))
    assert (O.tube_outward(pts, out) < 0).all()                                                 # the seed looks up: everything turns inwards


def test_plane_lattice(PC):
    pts, nrm = O.plane_lattice()
    out, flipped = check_cloud(PC, "plane", pts, nrm, 5)
    assert (out[:, 2] == 1).all() and np.array_equal(flipped, nrm[:, 2] < 0)


def test_moebius_cloud(PC):
    pts, nrm = O.moebius_cloud()
    check_cloud(PC, "moebius", pts, nrm, 10)


def test_two_tubes(PC):
    a, na = O.tube()
    b, nb = O.tube((0.0, 1.0, 0.0))
    pts, nrm = np.concatenate([a, b]), O.random_signs(np.concatenate([na, nb]), 7)
    out, _ = check_cloud(PC, "two tubes", pts, nrm, 10)
    assert PC.last_components == 2 and same_bits(out, np.concatenate([na, nb]))


def test_bad_rows(PC):
    pts, nrm, rows = O.bad_rows_tube()
    out, flipped = check_cloud(PC, "bad rows", pts, nrm, 10)
    assert same_bits(out[rows], nrm[rows]) and not flipped[rows].any()
    keep = np.setdiff1d(np.arange(len(pts)), rows)
    assert (O.tube_outward(pts[keep], out[keep]) > 0).all()


@pytest.mark.parametrize("n,k", [(1, 2), (2, 2), (2, 10), (257, 4), (257, 32), (5, 32)])
def test_small_counts(PC, n, k):
    pts, nrm = O.tube()
    start = O.random_signs(nrm, 5)
    check_cloud(PC, ("first", n), pts[:n], start[:n], k)


def test_all_invalid_and_fp64_and_tensors(PC):
    pts, nrm = O.tube()
    pts, nrm = pts[:300], O.random_signs(nrm, 5)[:300]
    zero = np.zeros_like(nrm)
    out, flipped = check_cloud(PC, "zero normals", pts, zero, 10)
    assert PC.last_components == 0 and not flipped.any()
    want = ref(("first", 300), O.orient_normals, pts, nrm, 10)
    got = PC.orient_normals_consistent_tangent_plane(torch.from_numpy(pts).cuda().double(), torch.from_numpy(nrm).double(), 10)
    assert same_bits(got[0].cpu().numpy(), want[0]) and np.array_equal(got[1].cpu().numpy(), want[1])


def test_repeat_and_method(PC):
    from bodyslam_amd.tsdf import PointCloud
    pts, nrm = O.moebius_cloud()
    a = PC.orient_normals_consistent_tangent_plane(pts, nrm, 10)
    b = PC.orient_normals_consistent_tangent_plane(pts, nrm, 10)
    assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)) and torch.equal(a[1], b[1])
    cloud = PointCloud(pts, None, nrm.copy())
    got = cloud.orient_normals_consistent_tangent_plane(10)
    assert isinstance(got, np.ndarray) and got is cloud.normals and same_bits(got, a[0].cpu().numpy())


# ---- meshes ------------------------------------------------------------------------------------------------------------------------------
def check_mesh(M, name, v, t, slots=None):
    want = ref(name, O.orient_triangles, v, t)
    out, flipped, ok = M.orient_triangles(v, t, slots=slots)
    assert out.is_cuda and out.dtype == torch.int32 and flipped.dtype == torch.bool and isinstance(ok, bool)
    assert M.last_orient_rounds >= (1 if len(t) else 0)
    out, flipped = out.cpu().numpy(), flipped.cpu().numpy()
    assert np.array_equal(flipped, want[1]), (name, int((flipped != want[1]).sum()))
    assert same_bits(out, want[0]) and ok == want[2], name
    comp, verdict = M.orientable_components(v, t, slots=slots)
    assert same_bits(comp.cpu().numpy(), want[3]) and np.array_equal(verdict.cpu().numpy(), want[4]), name
    assert M.is_orientable(v, t, slots=slots) == want[2]
    return out, flipped, ok


def flipped_torus():
    v, t = O.torus()
    rows = np.nonzero(np.random.default_rng(1).random(len(t)) < 1 / 3)[0]
    return v, O.flip_rows(t, rows), t, rows


@pytest.mark.parametrize("factor", [None, 4])
def test_closed_surface(M, factor):
    v, t, good, rows = flipped_torus()
    slots = None if factor is None else factor * M.edge_table_slots(len(t))
    assert not M.edge_topology(v, t).is_consistently_oriented()
    out, flipped, ok = check_mesh(M, "torus", v, t, slots)
    assert ok and not flipped[0] and M.edge_topology(v, out).is_consistently_oriented()
    assert same_bits(out, good if 0 not in rows else O.flip_rows(good, np.arange(len(good))))   # wound like triangle 0


def test_moebius_strip(M):
    v, t = O.moebius_strip()
    out, flipped, ok = check_mesh(M, "moebius strip", v, t)
    assert not ok and same_bits(out, t) and not flipped.any()


def test_strip_and_torus_in_one_mesh(M):
    v, t, good, _ = flipped_torus()
    sv, st = O.moebius_strip()
    mv, mt = O.merged((sv, st), (v, t))
    out, flipped, ok = check_mesh(M, "strip and torus", mv, mt)
    comp, verdict = M.orientable_components(mv, mt)
    assert not ok and verdict.cpu().tolist() == [False, True] and comp.cpu().tolist() == [0] * 32 + [1] * 384
    assert same_bits(out[:32], st) and not flipped[:32].any() and flipped[32:].any()
    assert M.edge_topology(v, out[32:] - len(sv)).is_consistently_oriented()


def test_three_triangles_on_one_edge(M):
    v, t = O.book()
    out, flipped, ok = check_mesh(M, "book", v, t)
    assert ok and not flipped[[0, 2, 4]].any() and M.orientable_components(v, t)[0].cpu().tolist() == [0, 0, 1, 1, 2, 2]


def test_invalid_triangles_and_empty(M):
    v, t, _, _ = flipped_torus()
    t = t.copy()
    t[5] = [3, 3, 7]
    t[100] = [0, 1, len(v)]
    t[383] = [-1, 2, 3]
    out, flipped, ok = check_mesh(M, "torus with invalid rows", v, t)
    assert same_bits(out[[5, 100, 383]], t[[5, 100, 383]]) and not flipped[[5, 100, 383]].any()
    assert M.orientable_components(v, t)[0].cpu()[[5, 100, 383]].tolist() == [-1, -1, -1]
    junk = np.array([[0, 0, 1], [5, 6, 999]], np.int32)
    out, flipped, ok = check_mesh(M, "only invalid rows", v, junk)
    assert ok and same_bits(out, junk)
    out, flipped, ok = M.orient_triangles(v, np.zeros((0, 3), np.int32))
    assert tuple(out.shape) == (0, 3) and flipped.numel() == 0 and ok and M.last_orient_rounds == 0
    assert M.is_orientable(v, np.zeros((0, 3), np.int32))


def test_long_strip(M):
    from bodyslam_amd.tsdf import TriangleMesh
    v, t, good = O.long_strip()
    out, flipped, ok = check_mesh(M, "long strip", v, t)
    assert ok and M.last_orient_rounds > 1 and M.edge_topology(v, out).is_consistently_oriented()
    mesh = TriangleMesh(v, None, t)
    assert mesh.is_orientable() and not mesh.is_consistently_oriented()
    new, f, ok = mesh.orient_triangles()
    assert isinstance(new.triangles, np.ndarray) and same_bits(new.triangles, out) and np.array_equal(f, flipped) and ok
    assert new.is_consistently_oriented()
