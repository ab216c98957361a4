"""The counting queries of the triangle-mesh scene without a GPU: the numpy statement (tests/_mesh_hits_ref.py) where the answer is known
in closed form -- the parity of a count inside and outside a cube whose triangles lie in dyadic planes, rays from the centre of an icosphere
through each of its vertices --, the grid walk against brute force, and the public interface (signatures, argument validation)."""
import inspect
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _mesh_hits_ref as H  # noqa: E402
import _mesh_scene_ref as M  # noqa: E402

f32 = np.float32


rays_from, edge_rays = H.rays_from, H.edge_rays


def test_the_tie_rule_decides_every_parity_of_the_cube_lattice():
    scene = M.Scene(M.cube())
    pts, inside = H.cube_lattice()
    assert len(pts) == 1811 and inside.sum() == 343
    for d in H.PARITY_DIRECTIONS:
        rays = rays_from(pts, d)
        odd = (H.count_intersections(scene, rays) & 1).astype(bool)
        closed = (H.count_intersections(scene, rays, tie=False) & 1).astype(bool)
        assert np.array_equal(odd, inside), (d, int((odd != inside).sum()))
        assert (closed != inside).any(), d                    # the predicate of the nearest hit cannot be used for a parity


def test_one_triangle_of_a_fan_claims_a_ray_through_its_vertex():
    v, t = M.icosphere(2)
    scene = M.Scene((v, t))
    rays = np.concatenate([np.zeros_like(v), v], 1)
    assert len(v) == 162 and (H.count_intersections(scene, rays) == 1).all()
    closed = H.count_intersections(scene, rays, tie=False)
    assert set(np.unique(closed)) == {1, 5, 6}
    assert H.test_occlusions(scene, rays).all()
    assert np.array_equal(H.compute_occupancy(scene, v * f32(0.5)), np.ones(162, f32))


def test_without_ties_the_predicate_is_the_closed_one():
    scene = M.Scene(M.cube())
    rays = np.concatenate([edge_rays(), rays_from(np.random.default_rng(0).uniform(-1.4, 1.4, (64, 3)).astype(f32), (0.3, 0.7, -0.2))])
    frame = M._ray_frame(rays)
    mine, ref = H.intersect(scene, *frame[:1], *frame[2:], tie=False), M._intersect(scene, *frame[:1], *frame[2:])
    for a, b in zip(mine, ref):
        assert np.array_equal(a, b, equal_nan=True)
    tie = H.intersect(scene, *frame[:1], *frame[2:], tie=True)
    assert not (tie[0] & ~ref[0]).any()                       # a tie only rejects
    assert np.array_equal(H.test_occlusions(scene, rays), np.isfinite(M.cast_rays(scene, rays)["t_hit"]))


def test_lists_are_sorted_and_agree_with_counts_and_the_nearest_hit():
    scene = M.Scene(M.cube(), M.icosphere(1))
    rng = np.random.default_rng(1)
    rays = np.concatenate([edge_rays(), np.concatenate([rng.uniform(-1.4, 1.4, (96, 3)), rng.normal(size=(96, 3))], 1).astype(f32)])
    ls, cnt = H.list_intersections(scene, rays), H.count_intersections(scene, rays)
    assert np.array_equal(np.diff(ls["ray_splits"]), cnt) and ls["ray_splits"][-1] == len(ls["t_hit"]) and cnt.max() >= 4
    assert np.array_equal(ls["ray_ids"], np.repeat(np.arange(len(rays)), cnt))
    near = M.cast_rays(scene, rays)
    for i in range(len(rays)):
        s = slice(ls["ray_splits"][i], ls["ray_splits"][i + 1])
        key = list(zip(ls["t_hit"][s], ls["global_ids"][s]))
        assert key == sorted(key)
        if i >= len(edge_rays()) and cnt[i]:                  # random rays have no zero edge value
            first = s.start
            assert ls["t_hit"][first] == near["t_hit"][i] and ls["primitive_ids"][first] == near["primitive_ids"][i]
            assert ls["geometry_ids"][first] == near["geometry_ids"][i] and np.array_equal(ls["primitive_uvs"][first], near["primitive_uvs"][i])
    # tnear, tfar equal to a hit's t exactly: both ends are closed
    i = len(edge_rays()) + int(np.argmax(cnt[len(edge_rays()):] >= 2))
    t = ls["t_hit"][ls["ray_splits"][i]:ls["ray_splits"][i + 1]]
    assert H.count_intersections(scene, rays[i:i + 1], tnear=t[0], tfar=t[1])[0] == 2 + int((t[2:] == t[1]).sum())
    assert H.count_intersections(scene, rays[i:i + 1], tnear=np.nextafter(t[0], f32(np.inf)), tfar=np.nextafter(t[1], f32(0)))[0] == 0 or t[0] == t[1]


@pytest.mark.parametrize("cell", [None, 0.3, 1.1])
def test_the_grid_walk_meets_every_hit_exactly_once(cell):
    scene = M.Scene(M.cube(), M.icosphere(1))
    grid = M.Grid(scene, cell)
    rng = np.random.default_rng(2)
    rays = np.concatenate([edge_rays(), np.concatenate([rng.uniform(-1.6, 1.6, (48, 3)), rng.normal(size=(48, 3))], 1).astype(f32),
                           rays_from(H.cube_lattice()[0][::40], (1, 1, 0))])
    stats = {}
    assert np.array_equal(H.count_intersections_grid(grid, rays, stats_out=stats), H.count_intersections(scene, rays))
    assert stats["fallback"] == 2 and stats["tests"] < len(rays) * len(scene.v0)
    a, b = H.list_intersections_grid(grid, rays), H.list_intersections(scene, rays)
    for k in b:
        assert np.array_equal(a[k].view(np.uint32) if a[k].dtype == f32 else a[k], b[k].view(np.uint32) if b[k].dtype == f32 else b[k]), k
    assert np.array_equal(H.test_occlusions_grid(grid, rays), H.test_occlusions(scene, rays))
    for tn, tf in ((0.5, 2.0), (2.0, 2.0), (2.5, np.inf)):    # (2.0: the first hit of the rays from z = -3)
        assert np.array_equal(H.count_intersections_grid(grid, rays, tn, tf), H.count_intersections(scene, rays, tn, tf))
        assert np.array_equal(H.test_occlusions_grid(grid, rays, tn, tf), H.test_occlusions(scene, rays, tn, tf))


def test_occupancy_and_signed_distance_of_the_statement():
    scene = M.Scene(M.cube())
    pts, inside = H.cube_lattice()
    pts, inside = pts[::7], inside[::7]
    for n in (1, 5):
        assert np.array_equal(H.compute_occupancy(scene, pts, n), inside.astype(f32))
    q = np.concatenate([pts[:8], [[np.nan, 0, 0]]]).astype(f32)
    sd, d = H.compute_signed_distance(scene, q), M.closest_points(scene, q)["distance"]
    assert np.isnan(sd[-1]) and np.isnan(H.compute_occupancy(scene, q)[-1])
    assert np.array_equal(np.abs(sd[:8]), d[:8]) and np.array_equal(sd[:8] < 0, inside[:8])
    assert np.array_equal(H.compute_signed_distance(M.Scene(), pts[:4]), np.full(4, np.inf, f32))
    assert (H.compute_signed_distance(scene, np.zeros((1, 3), f32)) == f32(-1)).all()


# ---- the public interface ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    import bodyslam_amd.evaluation as EV
    import bodyslam_amd.raycasting as RC
    import bodyslam_amd.tsdf as TS
    return RC, EV, TS


def test_public_signatures(built):
    RC, EV, TS = built

    def params(fn):
        return [(p.name, p.default) for p in inspect.signature(fn).parameters.values()]
    E, S, inf = inspect.Parameter.empty, RC.RaycastingScene, float("inf")
    assert params(S.count_intersections) == [("self", E), ("rays", E), ("method", "grid")]
    assert params(S.list_intersections) == [("self", E), ("rays", E), ("method", "grid")]
    assert params(S.test_occlusions) == [("self", E), ("rays", E), ("tnear", 0.0), ("tfar", inf), ("method", "grid")]
    assert params(S.compute_occupancy) == [("self", E), ("query", E), ("nsamples", 1), ("method", "grid")]
    assert params(S.compute_signed_distance) == [("self", E), ("query", E), ("nsamples", 1), ("method", "grid")]
    assert params(EV.evaluate_reconstruction_signed) == [("pred", E), ("gt", E), ("thresholds", (0.001, 0.002, 0.005)), ("transform", None),
                                                         ("max_distance", None), ("align", None), ("icp", None), ("n_gt_samples", None),
                                                         ("nsamples", 1)]
    assert [f.name for f in __import__("dataclasses").fields(EV.SignedReconstructionMetrics)] == [
        "surface", "n_inside", "n_outside", "fraction_inside", "inside", "outside", "signed_mean"]
    assert np.array_equal(np.array(RC.OCCUPANCY_DIRECTIONS, f32), H.DIRECTIONS)
    from bodyslam_amd import _lib as L
    assert (L.MESH_HITS_COUNT, L.MESH_HITS_ANY, L.MESH_HITS_FILL) == (H.COUNT, H.ANY, H.FILL)
    not_built = RC.__doc__.split("Not built")[1]
    assert "BVH" in not_built and "pinhole" in not_built
    for gone in ("occlusion", "count_intersections", "list_intersections", "signed distance", "occupancy"):
        assert gone not in not_built
    for fn in (S.compute_occupancy, S.compute_signed_distance, EV.evaluate_reconstruction_signed):
        assert "closed" in fn.__doc__.lower() and "edge-on" in fn.__doc__
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    head = open(os.path.join(root, "bodyslam_amd", "csrc", "mesh_scene.hip")).read().split("#include")[0]
    assert "tests/_mesh_hits_ref.py" in head and "UNPINNED" in head.split("Counting (")[1]
    design = open(os.path.join(root, "DESIGN.md")).read()
    assert "3.25" in design and "UNPINNED" in design.split("3.25")[1]


def test_argument_validation(built):
    RC, EV, TS = built
    for n in (0, 2, 4, 16, 17, -1, 1.0, True, "1", None):
        with pytest.raises(ValueError):
            RC._check_nsamples(n)
    assert [RC._check_nsamples(n) for n in (1, 3, 15)] == [1, 3, 15]
    for bad in ((np.nan, 1.0), (0.0, np.nan), ("0", 1.0), (0.0, None), (True, 1.0)):
        with pytest.raises(ValueError):
            RC._check_range(*bad)
    assert RC._check_range(0, np.inf) == (0.0, float("inf")) and RC._check_range(0.1, 2) == (float(f32(0.1)), 2.0)
    v, t = M.cube()
    mesh = TS.TriangleMesh(v, np.zeros_like(v), t)
    pred = (v * f32(0.9)).astype(f32)
    # everything but the closedness of the mesh (a device query) is checked before the GPU is touched
    for kw in (dict(gt=v), dict(gt=TS.PointCloud(v, v)), dict(nsamples=2), dict(nsamples=17), dict(nsamples=1.0), dict(n_gt_samples=0),
               dict(thresholds=(1,) * 9), dict(align="icp"), dict(icp=dict(max_correspondence_distance=0.01)), dict(gt=TS.TriangleMesh(v, v, t[:0]))):
        args = dict(pred=pred, gt=mesh)
        args.update(kw)
        with pytest.raises(ValueError):
            EV.evaluate_reconstruction_signed(**args)
    if not torch.cuda.is_available():                         # no CPU fallback
        from bodyslam_amd._lib import BodySlamHipError
        with pytest.raises(BodySlamHipError):
            EV.evaluate_reconstruction_signed(pred, mesh)
