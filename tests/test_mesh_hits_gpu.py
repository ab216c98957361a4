"""The counting queries of the triangle-mesh scene on the device against the numpy statement (tests/_mesh_hits_ref.py): counts, lists and
occlusion, equal for both methods and three cell sizes, on a cube, an icosphere, an open height field and a scene of two geometries; the
invariants that tie them to cast_rays; occupancy, signed distance and the signed reconstruction evaluation; degenerate scenes."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _mesh_hits_ref as H  # noqa: E402
import _mesh_scene_ref as M  # noqa: E402

pytestmark = pytest.mark.gpu
f32 = np.float32
LIST_KEYS = ("ray_splits", "ray_ids", "t_hit", "geometry_ids", "primitive_ids", "primitive_uvs")


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=f32)).view(np.uint32)


@pytest.fixture(scope="module")
def RC():
    import bodyslam_amd.raycasting as RC
    return RC


def random_rays(seed, n, reach):
    rng = np.random.default_rng(seed)
    return np.concatenate([rng.uniform(-reach, reach, (n, 3)), rng.normal(size=(n, 3))], 1).astype(f32)


def _cube():
    # every special ray, random rays from inside and around, a slice of the lattice along a face diagonal (edges and vertices all the way)
    return (M.cube(),), np.concatenate([H.edge_rays(), random_rays(3, 400, 1.6), H.rays_from(H.cube_lattice()[0][::6], (1, 1, 0))]), (None, 0.3, 1.1)


def _sphere():
    v, t = M.icosphere(2)
    return ((v, t),), np.concatenate([np.concatenate([np.zeros_like(v), v], 1), np.concatenate([-2 * v, v], 1), random_rays(4, 300, 1.2)]), (None, 0.15, 0.9)


def _field():
    v, t = M.height_field()
    rng = np.random.default_rng(5)
    o = np.concatenate([rng.uniform(-0.07, 0.07, (300, 2)), rng.uniform(0.25, 0.4, (300, 1))], 1)          # (the surface: z in 0.30 .. 0.34)
    down = np.concatenate([v[::19, :2], np.full((len(v[::19]), 1), 0.5)], 1)           # straight down onto lattice vertices
    rays = np.concatenate([np.concatenate([o, rng.normal(size=(300, 3)) * [1, 1, 0.3]], 1), H.rays_from(down.astype(f32), (0, 0, -1)),
                           [[0, 0, 50, 0, 0, -1], [0, 0, 0, 0, 0, 0], [0, np.nan, 0, 0, 0, 1]]]).astype(f32)
    return ((v, t),), rays, (None, 0.004, 0.03)


def _pair():
    v, t = M.icosphere(1)
    return (M.cube(), ((v * f32(0.5) + f32(0.25)).astype(f32), t)), np.concatenate([H.edge_rays(), random_rays(6, 400, 1.6)]), (None, 0.3, 1.1)


SCENES = dict(cube=_cube, sphere=_sphere, field=_field, pair=_pair)
_cache = {}


def case(name):
    """(geometries, rays, cell sizes, the statement's count, list, occlusion and ranged results) -- computed once, never changed"""
    if name not in _cache:
        geometries, rays, cells = SCENES[name]()
        ref = M.Scene(*geometries)
        hit = H.hit_matrix(ref, rays, True)
        ranges = ((0.5, 2.0), (2.0, 2.0), (2.5, np.inf))                               # (2.0: the cube's first hit from z = -3, exactly)
        _cache[name] = dict(geometries=geometries, rays=rays, cells=cells, ref=ref, count=hit[0].sum(1).astype(np.int32),
                            list=H._rows(ref, rays, *hit), occluded=H.test_occlusions(ref, rays), ranges=ranges,
                            occluded_in=[H.test_occlusions(ref, rays, a, b) for a, b in ranges], near=M.cast_rays(ref, rays))
    return _cache[name]


def scene_of(RC, geometries, cell=None):
    s = RC.RaycastingScene(cell_size=cell)
    for g in geometries:
        s.add_triangles(*g)
    return s


def assert_list(got, ref, what):
    for k in LIST_KEYS:
        v = got[k]
        want = torch.int64 if k in ("ray_splits", "ray_ids") else (torch.int32 if k.endswith("_ids") else torch.float32)
        assert v.is_cuda and v.dtype == want, (what, k, v.dtype)
        a, b = v.cpu().numpy(), ref[k]
        a = a.view(np.uint32) if k.endswith("_ids") and k != "ray_ids" else a
        assert a.shape == b.shape, (what, k, a.shape, b.shape)
        same = (bits(a) == bits(b)) if a.dtype == f32 else (a == b)
        assert same.all(), f"{what}: {k}: {int((~same).sum())} of {a.size} differ, first at {np.argwhere(~same)[0]}"


@pytest.mark.parametrize("name", list(SCENES))
def test_counts_lists_and_occlusion_equal_the_statement(RC, name):
    c = case(name)
    rays = c["rays"]
    assert c["count"].max() >= (1 if name == "field" else 2) and c["occluded"].any() and not c["occluded"].all()
    for cell in c["cells"]:
        scene = scene_of(RC, c["geometries"], cell)
        for method in RC.METHODS:
            what = f"{name}, cell {cell}, {method}"
            count = scene.count_intersections(rays, method=method)
            assert count.is_cuda and count.dtype == torch.int32 and np.array_equal(count.cpu().numpy(), c["count"]), what
            if method == "grid":
                assert scene.last_fallback == dict(field=1, sphere=0).get(name, 2), what       # fallback rays mixed with grid rays in one call
            ls = scene.list_intersections(rays, method=method)
            assert_list(ls, c["list"], what)
            occ = scene.test_occlusions(rays, method=method)
            assert occ.dtype == torch.bool and np.array_equal(occ.cpu().numpy(), c["occluded"]), what
            for (a, b), ref in zip(c["ranges"], c["occluded_in"]):
                assert np.array_equal(scene.test_occlusions(rays, tnear=a, tfar=b, method=method).cpu().numpy(), ref), (what, a, b)
            # the invariants
            near = scene.cast_rays(rays, method=method)
            assert torch.equal(occ, torch.isfinite(near["t_hit"])), what
            assert torch.equal(torch.diff(ls["ray_splits"]), count.long()), what
            again = scene.list_intersections(rays, method=method)
            assert all(torch.equal(again[k].view(torch.int32) if again[k].dtype == torch.float32 else again[k],
                                   ls[k].view(torch.int32) if ls[k].dtype == torch.float32 else ls[k]) for k in LIST_KEYS), what
    if name in ("cube", "pair"):
        assert c["occluded_in"][1].any() and not np.array_equal(c["occluded_in"][1], c["occluded_in"][0])     # tnear = tfar = a hit's t


@pytest.mark.parametrize("name", ["cube", "field"])
def test_the_first_row_of_a_list_is_the_nearest_hit(RC, name):
    c = case(name)
    scene = scene_of(RC, c["geometries"])
    rays = random_rays(7, 600, 1.5 if name == "cube" else 0.06)                          # random rays: no edge value is exactly 0
    if name == "field":
        rays[:, 2] += f32(0.32)
    ls, near = scene.list_intersections(rays), scene.cast_rays(rays)
    first = ls["ray_splits"][:-1]
    some = torch.diff(ls["ray_splits"]) > 0
    assert int(some.sum()) > 50 and torch.equal(some, torch.isfinite(near["t_hit"]))
    f = first[some]
    assert torch.equal(ls["t_hit"][f].view(torch.int32), near["t_hit"][some].view(torch.int32))
    assert torch.equal(ls["primitive_uvs"][f].view(torch.int32), near["primitive_uvs"][some].view(torch.int32))
    assert torch.equal(ls["primitive_ids"][f], near["primitive_ids"][some]) and torch.equal(ls["geometry_ids"][f], near["geometry_ids"][some])


def test_leading_shapes_and_input_kinds(RC):
    c = case("cube")
    scene = scene_of(RC, c["geometries"])
    rays = c["rays"][:24].reshape(2, 3, 4, 6)
    count = scene.count_intersections(rays)
    assert tuple(count.shape) == (2, 3, 4) and np.array_equal(count.cpu().numpy().ravel(), c["count"][:24])
    assert tuple(scene.test_occlusions(torch.from_numpy(rays).cuda().double()).shape) == (2, 3, 4)
    assert tuple(scene.list_intersections(rays)["ray_splits"].shape) == (25,)
    assert tuple(scene.compute_occupancy(np.zeros((2, 5, 3))).shape) == (2, 5) and tuple(scene.compute_signed_distance(np.zeros((0, 3), f32)).shape) == (0,)
    assert tuple(scene.count_intersections(np.zeros((0, 6), f32)).shape) == (0,) and scene.list_intersections(np.zeros((0, 6), f32))["t_hit"].numel() == 0
    for call in (lambda: scene.count_intersections(rays, method="bvh"), lambda: scene.test_occlusions(rays, tnear=np.nan),
                 lambda: scene.compute_occupancy(np.zeros((1, 3), f32), nsamples=2), lambda: scene.compute_signed_distance(np.zeros((1, 3), f32), nsamples=17),
                 lambda: scene.list_intersections(np.zeros((4, 5), f32))):
        with pytest.raises(ValueError):
            call()


def test_a_row_longer_than_the_sorting_network(RC):
    # 40 concentric icosahedra: a ray through the middle has 80 hits, more than the 64 keys a wave sorts in registers
    v, t = M.icosphere(0)
    radii = np.linspace(0.2, 1.0, 40)
    geometry = (np.concatenate([v * f32(r) for r in radii]).astype(f32), np.concatenate([t + 12 * k for k in range(40)]).astype(np.int32))
    ref = M.Scene(geometry)
    rays = np.array([[-2, 0.013, 0.021, 1, 0, 0], [0.01, 0.02, 0.03, 0.2, 1, 0.1], [-2, -2, -2.1, 1, 1, 1], [2, 2, 2, 1, 0, 0]], f32)
    want = H.list_intersections(ref, rays)
    assert list(np.diff(want["ray_splits"])) == [80, 40, 80, 0]
    scene = scene_of(RC, (geometry,))
    for method in RC.METHODS:
        assert_list(scene.list_intersections(rays, method=method), want, method)


def test_occupancy_of_the_cube_and_the_sphere(RC):
    pts, inside = H.cube_lattice()
    scene = scene_of(RC, (M.cube(),))
    for n in (1, 5):
        for method in RC.METHODS:
            occ = scene.compute_occupancy(pts, nsamples=n, method=method)
            assert occ.is_cuda and occ.dtype == torch.float32 and np.array_equal(occ.cpu().numpy(), inside.astype(f32)), (n, method)
    rng = np.random.default_rng(8)
    q = (rng.normal(size=(3000, 3)) * 0.6).astype(f32)
    r = np.linalg.norm(q.astype(np.float64), axis=1)
    q, r = q[(r < 0.93) | (r > 1.01)], r[(r < 0.93) | (r > 1.01)]                        # the icosphere's faces lie between these radii
    sphere = scene_of(RC, (M.icosphere(2),))
    for n in (1, 3):
        assert np.array_equal(sphere.compute_occupancy(q, nsamples=n).cpu().numpy(), (r < 0.95).astype(f32)), n


def test_signed_distance_has_the_distance_bits_and_the_statement_signs(RC):
    pts, inside = H.cube_lattice()
    q = np.concatenate([pts[::5], [[np.nan, 0, 0], [0, np.inf, 0], [0, 0, 0]]]).astype(f32)
    ref = M.Scene(M.cube())
    scene = scene_of(RC, (M.cube(),))
    want = H.compute_signed_distance(ref, q, 3)
    for method in RC.METHODS:
        sd, d = scene.compute_signed_distance(q, nsamples=3, method=method).cpu().numpy(), scene.compute_distance(q, method=method).cpu().numpy()
        assert np.array_equal(bits(sd)[:-3], bits(want)[:-3]) and np.isnan(sd[-3:-1]).all() and sd[-1] == f32(-1)
        assert np.array_equal(bits(np.abs(sd)), bits(np.abs(d))) and np.array_equal(sd[:-3] < 0, inside[::5])
        assert np.array_equal(scene.compute_occupancy(q, 3, method=method).cpu().numpy(), H.compute_occupancy(ref, q, 3), equal_nan=True)


def test_degenerate_scenes(RC):
    rays = np.concatenate([H.edge_rays(), random_rays(9, 40, 1.5)])
    q = rays[:, :3]
    flat = (np.array([[0, 0, 0], [1, 1, 1], [2, 2, 2], [np.nan, 0, 0]], f32), np.array([[0, 1, 2], [0, 0, 1], [0, 1, 3]], np.int32))
    for geometries in ((), (flat,)):
        scene = scene_of(RC, geometries)
        for method in RC.METHODS:
            assert not scene.count_intersections(rays, method=method).any() and not scene.test_occlusions(rays, method=method).any()
            ls = scene.list_intersections(rays, method=method)
            assert ls["ray_splits"].shape == (len(rays) + 1,) and not ls["ray_splits"].any()
            assert all(ls[k].shape[0] == 0 for k in LIST_KEYS[1:]) and ls["primitive_uvs"].shape == (0, 2)
            finite = np.isfinite(q).all(1)
            occ, sd = scene.compute_occupancy(q, method=method).cpu().numpy(), scene.compute_signed_distance(q, method=method).cpu().numpy()
            assert (occ[finite] == 0).all() and np.isnan(occ[~finite]).all()
            assert (sd[finite] == np.inf).all() and np.isnan(sd[~finite]).all()
        assert scene.n_kept == 0


def test_signed_reconstruction_evaluation(RC):
    import bodyslam_amd.evaluation as EV
    import bodyslam_amd.tsdf as TS
    v, t = M.icosphere(2)
    mesh = TS.TriangleMesh(v, np.zeros_like(v), t)
    cloud = mesh.sample_points_uniformly(1500, seed=1, host=True)[0].points
    for scale, frac in ((0.98, 1.0), (1.02, 0.0)):
        pred = (cloud * f32(scale)).astype(f32)
        res = EV.evaluate_reconstruction_signed(pred, mesh)
        surface = EV.evaluate_reconstruction_surface(pred, mesh)
        a, b = res.surface.as_dict(), surface.as_dict()
        assert a.keys() == b.keys() and all(a[k] == b[k] or (a[k] != a[k] and b[k] != b[k]) for k in a)
        assert res.fraction_inside == frac and res.n_inside + res.n_outside == 1500 == surface.n_pred
        assert res.signed_mean == pytest.approx((1 - 2 * frac) * surface.accuracy.mean, rel=1e-12) and abs(res.signed_mean) > 0.005
        side, other = (res.inside, res.outside) if frac else (res.outside, res.inside)
        assert side.mean == surface.accuracy.mean and side.max == surface.accuracy.max and other.mean != other.mean
        d = res.as_dict()
        assert d["fraction_inside"] == frac and d["n_inside"] == res.n_inside and d["chamfer"] == surface.chamfer
    # the transform comes before the sign: the same cloud, put inside by a similarity
    T = np.diag([0.98, 0.98, 0.98, 1.0])
    assert EV.evaluate_reconstruction_signed(cloud, mesh, transform=T, nsamples=3).fraction_inside == 1.0
    cv, ct = M.cube()                                                                    # its faces share no vertex rows: not closed
    with pytest.raises(ValueError):
        EV.evaluate_reconstruction_signed(pred, TS.TriangleMesh(cv, np.zeros_like(cv), ct))
