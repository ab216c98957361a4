"""The triangle-mesh scene on the device against the numpy statement (tests/_mesh_scene_ref.py): every output of cast_rays,
compute_closest_points and sample_points_uniformly bit for bit -- pinhole views of a height-field mesh, special rays, ties, degenerate
scenes, far and on-surface query points, several seeds and batch sizes --, and the surface option of the reconstruction evaluation."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _mesh_scene_ref as M  # noqa: E402
import _pointcloud_ref as P  # noqa: E402
import _render as R  # noqa: E402

pytestmark = pytest.mark.gpu
f32 = np.float32


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=f32)).view(np.uint32)


def host(out):
    """a result dict of device tensors -> numpy, the ids as the uint32 the statement uses"""
    res = {}
    for k, v in out.items():
        assert v.is_cuda and v.dtype == (torch.int32 if k.endswith("_ids") else torch.float32), (k, v.dtype, v.device)
        a = v.cpu().numpy()
        res[k] = a.view(np.uint32) if k.endswith("_ids") else a
    return res


def assert_equals_statement(got, ref, what):
    got = host(got)
    for k, a in got.items():
        b = ref[k]
        assert a.shape == b.shape, (what, k, a.shape, b.shape)
        same = (a == b) if k.endswith("_ids") else (bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))
        wrong = np.argwhere(~same)
        assert len(wrong) == 0, f"{what}: {k}: {len(wrong)} of {a.size} differ, first at {tuple(wrong[0])}: device {a[tuple(wrong[0])]!r}, " \
                                f"statement {b[tuple(wrong[0])]!r}"
    return got


@pytest.fixture(scope="module")
def RC():
    import bodyslam_amd.raycasting as RC
    return RC


def scene_of(RC, *geometries):
    s = RC.RaycastingScene()
    for i, (v, t) in enumerate(geometries):
        assert s.add_triangles(v, t) == i
    return s


@pytest.fixture(scope="module")
def field(RC):
    v, t = M.height_field()
    return v, t, M.Scene((v, t)), scene_of(RC, (v, t))


@pytest.fixture(scope="module")
def cube(RC):
    v, t = M.cube()
    return v, t, M.Scene((v, t)), scene_of(RC, (v, t))


# ---- rays ------------------------------------------------------------------------------------------------------------------------------------
def test_pinhole_views_of_the_height_field(RC, field):
    v, t, ref_scene, scene = field
    assert scene.cast_rays(np.zeros((1, 6), f32))["t_hit"].shape == (1,) and scene.n_triangles == 5400 and scene.n_kept == 5400
    for i in (2, 5):
        pose = P.map_frames()[i][2]
        rays = RC.RaycastingScene.create_rays_pinhole(M.pinhole_matrix(P.MAP_K), np.linalg.inv(pose), P.MAP_W, P.MAP_H, pixel_center=0.0)
        got = assert_equals_statement(scene.cast_rays(rays), M.cast_rays(ref_scene, rays.numpy()), f"view {i}")
        assert got["t_hit"].shape == (P.MAP_H, P.MAP_W) and got["primitive_normals"].shape == (P.MAP_H, P.MAP_W, 3)
        hit = np.isfinite(got["t_hit"])
        assert hit.sum() > 300 and (got["geometry_ids"][hit] == 0).all() and (got["primitive_ids"][~hit] == M.INVALID).all()
        # t_hit IS the z-depth.  The tessellation error of the 2 mm mesh, measured with the statement: 1.67e-6 m (frame 2), 1.61e-6 m
        # (frame 5); the bound is twice the maximum (tests/test_mesh_scene_cpu.py asserts the same of the statement)
        assert np.abs(got["t_hit"][hit] - R.render(pose, P.MAP_K, P.MAP_H, P.MAP_W)[1][hit]).max() <= 2 * 1.67e-6
        # a device tensor of rays, and fp64 rays, give the same bits
        again = scene.cast_rays(rays.cuda())
        assert all(torch.equal(again[k], scene.cast_rays(rays.double())[k]) for k in again)
        assert np.array_equal(bits(again["t_hit"].cpu().numpy()), bits(got["t_hit"]))


def special_rays(v, t, lo, hi):
    """rays that lie in planes, edges and vertices of the mesh and of its box, from inside, from the boundary and from far away"""
    rng = np.random.default_rng(3)
    ext = (hi - lo).astype(np.float64)
    mid = (lo + hi) / 2
    inside = rng.uniform(lo + 0.1 * ext, hi - 0.1 * ext, (96, 3))
    on_box = inside.copy()
    axis = rng.integers(0, 3, 96)
    on_box[np.arange(96), axis] = np.where(rng.integers(0, 2, 96) == 0, lo[axis], hi[axis])
    far = mid + rng.normal(size=(96, 3)) / np.linalg.norm(rng.normal(size=(96, 3)), axis=1, keepdims=True) * 1e3 * ext.max()
    rays = []
    for o in (inside, on_box, far):
        target = v[rng.integers(0, len(v), len(o))].astype(np.float64)               # through lattice vertices
        rays.append(np.concatenate([o, target - o], 1))
        target = rng.uniform(lo, hi, (len(o), 3))
        rays.append(np.concatenate([o, target - o], 1))
    # axis-parallel rays that lie in the planes of the lattice and run along its edges, both ways, and with +0 / -0 components
    vert = v[rng.integers(0, len(v), 64)].astype(np.float64)
    for axis in range(3):
        for sign in (1.0, -1.0):
            d = np.zeros((64, 3))
            d[:, axis] = sign
            o = vert.copy()
            o[:, axis] -= sign * 2.0 * ext[axis]
            rays.append(np.concatenate([o, d], 1))
            rays.append(np.concatenate([o, np.where(d == 0, -0.0, d)], 1))
    rays = np.concatenate(rays).astype(f32)
    odd = np.array([[0, 0, 0, 0, 0, 0], [0, 0, 0, -0.0, 0, -0.0], [0, 0, 0, np.nan, 0, 1], [np.nan, 0, 0, 0, 0, 1], [0, 0, 0, np.inf, 0, 1],
                    [0, -np.inf, 0, 0, 0, 1], [0, 0, 0, 0, 0, np.inf]], f32)
    return rays, odd


@pytest.mark.parametrize("which", ["field", "cube"])
def test_special_rays(RC, field, cube, which):
    v, t, ref_scene, scene = field if which == "field" else cube
    rays, odd = special_rays(v, t, v.min(0), v.max(0))
    ref = M.cast_rays(ref_scene, rays)
    got = assert_equals_statement(scene.cast_rays(rays), ref, which)
    assert np.isfinite(got["t_hit"]).sum() > len(rays) // 4
    for length in (1e-3, 1e3):                                   # t scales with the direction's length
        scaled = rays.copy()
        scaled[:, 3:] *= f32(length)
        g = assert_equals_statement(scene.cast_rays(scaled), M.cast_rays(ref_scene, scaled), f"{which} x {length}")
        hit = np.isfinite(g["t_hit"]) & np.isfinite(got["t_hit"])                     # (a ray along an edge may change sides with the rounding)
        assert hit.sum() > 0.9 * np.isfinite(got["t_hit"]).sum()
        if which == "cube":                                      # a ray lying IN a face of the cube meets it edge-on, at no particular t:
            hit[192:] = False                                    # the rays from inside (the first 192) are the ones with a definite hit
        assert np.allclose(g["t_hit"][hit] * f32(length), got["t_hit"][hit], rtol=1e-4, atol=1e-6)
    g = assert_equals_statement(scene.cast_rays(odd), M.cast_rays(ref_scene, odd), f"{which} odd")
    assert np.isinf(g["t_hit"]).all() and (g["primitive_ids"] == M.INVALID).all() and not g["primitive_normals"].any()
    mixed = np.concatenate([odd, rays[::7], odd[::-1], rays[3::11]])
    mixed = mixed[:len(mixed) // 2 * 2]
    assert_equals_statement(scene.cast_rays(mixed.reshape(2, -1, 6)), M.cast_rays(ref_scene, mixed.reshape(2, -1, 6)), f"{which} mixed")


@pytest.mark.parametrize("which", ["field", "cube"])
def test_grid_equals_brute_at_three_cell_sizes(RC, field, cube, which):
    """method="grid" at the default cell size, half of it and three times it, and method="brute": all four identical, for rays and for
    closest points; every ray from 10^3 extents away and every point 0.5 m (the cube: 40 extents) away goes through the fallback"""
    v, t, ref_scene, scene = field if which == "field" else cube
    rays, odd = special_rays(v, t, v.min(0), v.max(0))
    pose = P.map_frames()[2][2]
    view = RC.RaycastingScene.create_rays_pinhole(M.pinhole_matrix(P.MAP_K), np.linalg.inv(pose), P.MAP_W, P.MAP_H, pixel_center=0.0).reshape(-1, 6).numpy()
    far = rays[384:576]                                          # the origins 10^3 extents away
    all_rays = torch.from_numpy(np.concatenate([rays, odd, view[::3], far[::5]])).cuda()
    src = P.base_source() if which == "field" else np.random.default_rng(7).uniform(-2, 2, (500, 3)).astype(f32)
    away = (src + f32(0.5 if which == "field" else 80.0)).astype(f32)
    q = torch.from_numpy(np.concatenate([src, away, v[::9], [[np.nan, 0, 0]]]).astype(f32)).cuda()
    brute_r, brute_c = scene.cast_rays(all_rays, method="brute"), scene.compute_closest_points(q, method="brute")
    brute_md = scene.compute_closest_points(q, max_distance=0.001, method="brute")
    scene.cast_rays(all_rays)
    h0 = scene.cell_size
    for mult in (1.0, 0.5, 3.0):
        s = RC.RaycastingScene(cell_size=None if mult == 1.0 else h0 * mult)
        s.add_triangles(v, t)
        got = s.cast_rays(all_rays)
        assert s.last_fallback == len(far) + len(far[::5]) and (mult == 1.0 or s.cell_size == float(f32(h0 * mult)))
        for k in got:
            assert torch.equal(got[k].view(torch.int32), brute_r[k].view(torch.int32)), (which, mult, k)
        s.cast_rays(torch.from_numpy(far).cuda())
        assert s.last_fallback == len(far)
        s.cast_rays(torch.from_numpy(rays[:384]).cuda())
        assert s.last_fallback == 0
        got = s.compute_closest_points(q)
        if which == "field":                                     # (the cube's grid is a few cells across: the shells reach all of it below the cap)
            assert s.last_fallback >= len(away)
            s.compute_closest_points(torch.from_numpy(away).cuda())
            assert s.last_fallback == len(away)
        for k in got:
            assert torch.equal(got[k].view(torch.int32), brute_c[k].view(torch.int32)), (which, mult, k)
        got = s.compute_closest_points(q, max_distance=0.001)
        for k in got:
            assert torch.equal(got[k].view(torch.int32), brute_md[k].view(torch.int32)), (which, mult, k, "max_distance")


def test_reference_cap(RC):
    """2 048 triangles that each span the box in x and y: the first guess of the cell size breaks the cap of max(8 T, 2^16) references, so
    the default grows and the same size given explicitly is refused; so is a size that needs more than 2^24 cells"""
    n = 2048
    z = np.linspace(0, 1, n)
    v = np.stack([np.tile([0.0, 1.0, 0.0], n), np.tile([0.0, 0.0, 1.0], n), np.repeat(z, 3)], 1).astype(f32)
    t = np.arange(3 * n, dtype=np.int32).reshape(n, 3)
    rays = np.concatenate([np.tile([0.3, 0.3, -1.0], (16, 1)), np.random.default_rng(6).normal(size=(16, 3)) * 0.1 + [0, 0, 1]], 1).astype(f32)
    s = scene_of(RC, (v, t))
    got = s.cast_rays(rays)
    first = P.default_cell_size(v.min(0), v.max(0), n)
    assert s.cell_size > first and s.n_references <= RC.max_references(n) == 2 ** 16
    assert_equals_statement(got, M.cast_rays(M.Scene((v, t)), rays), "slabs")
    for bad in (first, 1e-4):
        with pytest.raises(ValueError):
            b = RC.RaycastingScene(cell_size=bad)
            b.add_triangles(v, t)
            b.cast_rays(rays)


def test_cube_from_the_centre_hits_everywhere(RC, cube):
    v, t, ref_scene, scene = cube
    mids = np.concatenate([(v[t[:, a]] + v[t[:, b]]) / 2 for a, b in ((0, 1), (1, 2), (2, 0))])
    d = np.concatenate([v, mids, np.random.default_rng(0).normal(size=(4096, 3))]).astype(f32)
    rays = np.concatenate([np.zeros_like(d), d], 1)
    got = assert_equals_statement(scene.cast_rays(rays), M.cast_rays(ref_scene, rays), "cube")
    assert np.isfinite(got["t_hit"]).all() and np.array_equal(got["t_hit"][:len(v) + len(mids)], np.ones(len(v) + len(mids), f32))


def test_ties(RC):
    v, t = M.grid_patch(np.linspace(-1, 1, 5), np.linspace(-1, 1, 5), lambda X, Y: np.ones_like(X))
    d = np.concatenate([np.random.default_rng(2).uniform(-0.9, 0.9, (256, 2)), np.ones((256, 1))], 1).astype(f32)
    rays = np.concatenate([np.zeros_like(d), d], 1)
    q = (d * f32(1.5)).astype(f32)
    one = host(scene_of(RC, (v, t)).cast_rays(rays))
    tt = np.concatenate([t, t])
    twice = scene_of(RC, (v, tt))                                                   # the patch twice in one geometry: the lower row
    g = assert_equals_statement(twice.cast_rays(rays), M.cast_rays(M.Scene((v, tt)), rays), "twice")
    assert np.array_equal(g["primitive_ids"], one["primitive_ids"]) and (g["primitive_ids"] < len(t)).all()
    c = assert_equals_statement(twice.compute_closest_points(q), without_d2(M.closest_points(M.Scene((v, tt)), q)), "twice, closest")
    assert (c["primitive_ids"] < len(t)).all()
    two = scene_of(RC, (v, t), (v, t))                                              # as two geometries: geometry 0
    g = assert_equals_statement(two.cast_rays(rays), M.cast_rays(M.Scene((v, t), (v, t)), rays), "two")
    assert not g["geometry_ids"].any() and np.array_equal(g["primitive_ids"], one["primitive_ids"])
    c = assert_equals_statement(two.compute_closest_points(q), without_d2(M.closest_points(M.Scene((v, t), (v, t)), q)), "two, closest")
    assert not c["geometry_ids"].any()
    near = scene_of(RC, (v + f32(1), t), (v, t))                                     # the nearer geometry wins whatever its id; a later add rebuilds
    g = assert_equals_statement(near.cast_rays(rays), M.cast_rays(M.Scene((v + f32(1), t), (v, t)), rays), "near")
    assert (g["geometry_ids"] == 1).all()
    assert near.add_triangles(v - f32(0.5), t) == 2
    g = assert_equals_statement(near.cast_rays(rays), M.cast_rays(M.Scene((v + f32(1), t), (v, t), (v - f32(0.5), t)), rays), "near + 1")
    assert (g["geometry_ids"] == 2).sum() > 100


def without_d2(ref):
    return {k: v for k, v in ref.items() if k != "d2"}


def test_degenerate_scenes(RC):
    from bodyslam_amd.tsdf import TriangleMesh
    v, t = M.grid_patch(np.linspace(-1, 1, 5), np.linspace(-1, 1, 5), lambda X, Y: np.ones_like(X))
    d = np.concatenate([np.random.default_rng(2).uniform(-1.2, 1.2, (200, 2)), np.ones((200, 1))], 1).astype(f32)
    rays = np.concatenate([np.zeros_like(d), d], 1)
    q = np.concatenate([d * f32(2), [[np.nan, 0, 0]]]).astype(f32)
    # an empty scene
    empty = RC.RaycastingScene()
    assert_equals_statement(empty.cast_rays(rays), M.cast_rays(M.Scene(), rays), "empty")
    c = assert_equals_statement(empty.compute_closest_points(q), without_d2(M.closest_points(M.Scene(), q)), "empty, closest")
    assert np.isinf(c["distance"][:-1]).all() and np.isnan(c["distance"][-1])
    assert empty.cast_rays(np.zeros((0, 6), f32))["t_hit"].shape == (0,) and empty.compute_distance(np.zeros((0, 3), f32)).shape == (0,)
    # a single triangle, as a TriangleMesh
    tri = TriangleMesh(np.array([[0, 0, 1], [1, 0, 1], [0, 1, 1]], f32), np.zeros((3, 3), f32), np.array([[0, 1, 2]], np.int32))
    single, ref_single = RC.RaycastingScene(), M.Scene((tri.vertices, tri.triangles))
    assert single.add_triangles(tri) == 0
    g = assert_equals_statement(single.cast_rays(rays), M.cast_rays(ref_single, rays), "single")
    assert 0 < np.isfinite(g["t_hit"]).sum() < len(rays)
    assert_equals_statement(single.compute_closest_points(q), without_d2(M.closest_points(ref_single, q)), "single, closest")
    # a zero-area triangle and one with a NaN vertex among valid ones are never reported; fp64 vertices, int64 torch triangles
    vv = np.concatenate([v, [[np.nan, 0, 1], [0, 0, 0.5], [0.5, 0.5, 0.5], [1, 1, 0.5]]]).astype(f32)
    n = len(v)
    tt = np.concatenate([[[0, 1, n], [n + 1, n + 2, n + 3], [3, 3, 3]], t]).astype(np.int64)
    scene, ref_scene = scene_of(RC, (vv.astype(np.float64), torch.from_numpy(tt))), M.Scene((vv, tt))
    g = assert_equals_statement(scene.cast_rays(rays), M.cast_rays(ref_scene, rays), "degenerate rows")
    assert scene.n_triangles == len(tt) and scene.n_kept == len(t) and (g["primitive_ids"][np.isfinite(g["t_hit"])] >= 3).all()
    c = assert_equals_statement(scene.compute_closest_points(q), without_d2(M.closest_points(ref_scene, q)), "degenerate rows, closest")
    assert (c["primitive_ids"][:-1] >= 3).all()
    only = scene_of(RC, (vv, tt[:3]))                                                # nothing kept at all
    assert only.n_kept == 0 and np.isinf(host(only.cast_rays(rays))["t_hit"]).all()
    assert np.isinf(only.compute_distance(q[:-1]).cpu().numpy()).all()
    # one floor triangle under the patch that spans far beyond it
    floor = (np.array([[-50, -50, 0.5], [50, -50, 0.5], [0, 80, 0.5]], f32), np.array([[0, 1, 2]], np.int32))
    both, ref_both = scene_of(RC, (v, t), floor), M.Scene((v, t), floor)
    g = assert_equals_statement(both.cast_rays(rays), M.cast_rays(ref_both, rays), "floor")
    # (the floor's coordinates reach 80: half an ulp there is 3.8e-6, and a ray whose dominant axis is x or y shears with them)
    assert (g["geometry_ids"] == 1).all() and np.abs(g["t_hit"] - 0.5).max() < 4 * 3.8e-6
    assert_equals_statement(both.compute_closest_points(q), without_d2(M.closest_points(ref_both, q)), "floor, closest")
    # an index outside [0, V) is refused where the data is, before any kernel follows it
    for bad in (np.array([[0, 1, n]]), np.array([[0, -1, 2]])):
        with pytest.raises(ValueError):
            RC.RaycastingScene().add_triangles(v, bad)
        with pytest.raises(ValueError):
            RC.RaycastingScene().add_triangles(torch.from_numpy(v).cuda(), torch.from_numpy(bad).cuda())
    for bad in (dict(method="dda"), dict(method=None)):
        with pytest.raises(ValueError):
            single.cast_rays(rays, **bad)
        with pytest.raises(ValueError):
            single.compute_distance(q, **bad)
    with pytest.raises(ValueError):
        single.compute_closest_points(q, max_distance=-1.0)
    with pytest.raises(ValueError):
        single.cast_rays(q)


# ---- closest points --------------------------------------------------------------------------------------------------------------------------
def test_closest_points(RC, field, cube):
    v, t, ref_scene, scene = field
    src = P.base_source()
    assert len(src) == 1937
    edges = ((v[t[::23, 0]].astype(np.float64) + v[t[::23, 1]]) / 2).astype(f32)
    nan_rows = np.array([[np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf]], f32)
    near = src[:64] + np.array([0, 0, 0.00102], f32)                                     # about 1 mm off the surface: either side of max_distance
    q = np.concatenate([src, src + f32(0.5), v[::11], edges, nan_rows, near])
    ref = M.closest_points(ref_scene, q)
    got = assert_equals_statement(scene.compute_closest_points(q), without_d2(ref), "closest")
    assert np.array_equal(bits(got["distance"]), bits(np.sqrt(ref["d2"])))
    assert not got["distance"][2 * len(src):2 * len(src) + len(v[::11])].any()                      # on vertices: exactly 0
    assert np.isnan(got["distance"][-67:-64]).all() and (got["primitive_ids"][-67:-64] == M.INVALID).all()
    assert got["distance"][len(src):2 * len(src)].min() > 0.3
    d = scene.compute_distance(q.reshape(-1, 1, 3).astype(np.float64))
    assert d.shape == (len(q), 1) and np.array_equal(bits(d.cpu().numpy().ravel()), bits(got["distance"]))
    # max_distance = 1 mm, compared with the fp32 distance
    part = np.concatenate([q[5:2 * len(src):8], q[-67:]])
    ref_md = M.closest_points(ref_scene, part, max_distance=0.001)
    md = assert_equals_statement(scene.compute_closest_points(part, max_distance=0.001), without_d2(ref_md), "max_distance")
    cut, k = np.isinf(md["distance"]), len(q[5:len(src):8])
    assert not cut[:k].any() and cut[k:-67].all() and 0 < cut[-64:].sum() < 64 and np.isnan(md["points"][cut]).all()
    # the cube's closed forms
    v, t, ref_scene, scene = cube
    q = np.array([[2, 0.25, 0.25], [0.5, -3, 0.5], [2, 2, 2], [-1.5, 0.375, 3], [0, 0, 0], [0.25, 0.5, 0.75], [1, 1, 1], [0.5, 1, 0.25]], f32)
    got = assert_equals_statement(scene.compute_closest_points(q), without_d2(M.closest_points(ref_scene, q)), "cube")
    assert np.array_equal(got["distance"], np.sqrt(np.array([1, 4, 3, 4.25, 1, 0.0625, 0, 0], f32)))
    assert np.array_equal(got["points"][:4], np.array([[1, 0.25, 0.25], [0.5, -1, 0.5], [1, 1, 1], [-1, 0.375, 1]], f32))


# ---- sampling --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [0, 2 ** 63 + 12345])
def test_sampling_equals_the_statement(seed):
    import bodyslam_amd.pointcloud as PC
    from bodyslam_amd.tsdf import PointCloud, TriangleMesh
    v, t = M.height_field()
    v = np.concatenate([v, [[np.nan, 0, 0]]]).astype(f32)
    t = np.concatenate([t, [[0, 1, len(v) - 1], [5, 5, 6]]]).astype(np.int32)              # with a NaN and a zero-area triangle
    col = np.random.default_rng(4).uniform(0, 1, v.shape).astype(f32)
    mesh = TriangleMesh(v, col, t)
    for n in (1, 63, 64, 65, 4099):
        ref = M.sample_mesh(v, t, n, seed=seed, vertex_colors=col)
        cloud, idx = mesh.sample_points_uniformly(n, seed=seed)
        assert isinstance(cloud, PointCloud) and isinstance(cloud.points, np.ndarray) and idx.dtype == np.int32
        for name, a, b in (("points", cloud.points, ref[0]), ("colors", cloud.colors, ref[1]), ("normals", cloud.normals, ref[2])):
            assert a.shape == (n, 3) and np.array_equal(bits(a), bits(b)), (name, n)
        assert np.array_equal(idx, ref[3]) and idx.max() < 5400
        again, idx2 = mesh.sample_points_uniformly(n, seed=seed, host=False)              # a second run: the same bits, on the device
        assert again.points.is_cuda and np.array_equal(bits(again.points.cpu().numpy()), bits(ref[0])) and np.array_equal(idx2.cpu().numpy(), ref[3])
    # a batch split, and no colours
    ref = M.sample_mesh(v, t, 4099, seed=seed)
    a = PC.sample_mesh(v, t, 1000, seed=seed)
    b = PC.sample_mesh(torch.from_numpy(v).cuda(), torch.from_numpy(t).cuda().long(), 3099, seed=seed, first=1000)
    assert a[1] is None and b[1] is None
    for k in (0, 2, 3):
        assert np.array_equal(np.concatenate([a[k].cpu().numpy(), b[k].cpu().numpy()]).view(np.uint32), np.ascontiguousarray(ref[k]).view(np.uint32))
    # no triangle of positive weight: an empty cloud
    e, ei = TriangleMesh(v, col, t[-2:]).sample_points_uniformly(16, seed=seed)
    assert e.points.shape == (0, 3) and e.colors.shape == (0, 3) and e.normals.shape == (0, 3) and ei.shape == (0,)
    with pytest.raises(ValueError):
        PC.sample_mesh(v, np.array([[0, 1, len(v)]]), 4)


def test_sampling_area_shares():
    import bodyslam_amd.pointcloud as PC
    v = np.array([[0, 0, 0], [3, 0, 0], [0, 2, 0], [5, 0, 0], [6, 0, 0], [5, 2, 0]], f32)
    t = np.array([[0, 1, 2], [3, 4, 5]], np.int32)                                        # areas 3 : 1
    n = 2 ** 16
    pts, _, nrm, idx = PC.sample_mesh(v, t, n, seed=0)
    ref = M.sample_mesh(v, t, n, seed=0)
    assert np.array_equal(bits(pts.cpu().numpy()), bits(ref[0])) and np.array_equal(idx.cpu().numpy(), ref[3])
    share = float((idx == 0).float().mean())
    assert abs(share - 0.75) <= 5 * np.sqrt(0.75 * 0.25 / n), share


# ---- the evaluation ------------------------------------------------------------------------------------------------------------------------
def test_evaluation_against_the_surface():
    import bodyslam_amd.evaluation as EV
    from bodyslam_amd.tsdf import TriangleMesh
    gv, gt = M.height_field(0.008)
    mesh = TriangleMesh(gv, np.zeros_like(gv), gt)
    pred = P.map_gt_samples()
    surf = EV.evaluate_reconstruction_surface(pred, mesh)
    vert = EV.evaluate_reconstruction(pred, mesh)
    # accuracy of true surface points against the 8 mm mesh, measured with the statement (M.closest_points, P.nn_brute): mean 1.17e-5 m to
    # the surface -- the mesh's own tessellation error -- against 3.08e-3 m to the vertices
    print("accuracy mean: surface", surf.accuracy.mean, "vertices", vert.accuracy.mean)
    assert surf.accuracy.mean <= vert.accuracy.mean / 10
    ref = M.closest_points(M.Scene((gv, gt)), pred)["distance"].astype(np.float64)
    assert surf.accuracy.mean == pytest.approx(ref.mean(), rel=1e-12) and surf.accuracy.max == float(ref.max())
    assert surf.n_pred == len(pred) and surf.n_gt == len(pred) and surf.completeness.mean < 0.003
    fewer = EV.evaluate_reconstruction_surface(pred, mesh, n_gt_samples=1000)
    assert fewer.n_gt == 1000 and fewer.accuracy == surf.accuracy
    # "vertices" is today's path: bit-identical to a call without the keyword
    same = EV.evaluate_reconstruction_surface(pred, mesh, gt_mesh="vertices")
    assert same.as_dict() == vert.as_dict()
    with pytest.raises(ValueError):
        EV.evaluate_reconstruction_surface(pred, gv)
    # ICP onto the surface samples and their face normals: from a 2 mm offset back to the true pose
    T = np.eye(4)
    T[:3, 3] = (0.0012, -0.0010, 0.0012)                                                # |t| = 2 mm
    moved = (pred.astype(np.float64) + T[:3, 3]).astype(f32)
    res = EV.evaluate_reconstruction_surface(moved, mesh, align="icp", icp=dict(max_correspondence_distance=0.01, estimation="point_to_plane"))
    got = res.alignment.transformation
    err = np.linalg.norm(moved.astype(np.float64) @ got[:3, :3].T + got[:3, 3] - pred.astype(np.float64), axis=1).max()
    print("icp:", got[:3, 3], "fitness", res.alignment.fitness, "largest distance to the true position", err, "accuracy mean", res.accuracy.mean)
    # the existing ICP test's tolerance on the recovered pose (tests/test_icp_cpu.py RECOVERY_BOUND: the largest distance between a
    # registered point and its true position); the statement (tests/_icp_ref.py on the statement's samples and face normals) measures 3.4e-5 m
    assert err <= 5e-5
    assert res.accuracy.mean <= surf.accuracy.mean + 5e-5            # (no point is further from where it was than err)


# ---- end to end: the mesh of a map, rendered ---------------------------------------------------------------------------------------------
def test_render_the_mesh_of_a_map(RC):
    """the eight-frame map of tests/test_pointcloud_gpu.py: its extract_mesh(), cast from frame 3's camera at pixel_center = 0, against
    TSDF.raycast of the same view and against the analytic renderer"""
    from bodyslam_amd.tsdf import TSDF, PinholeCameraIntrinsic, RGBDImage
    frames = P.map_frames()
    intr = PinholeCameraIntrinsic(P.MAP_W, P.MAP_H, *P.MAP_K)
    m = TSDF(P.MAP_VL, P.MAP_TRUNC, volume_unit_resolution=P.MAP_RES, depth_sampling_stride=P.MAP_STRIDE, slab_bytes=1 << 24, max_units=8192)
    for (col, dep, _), E in zip(frames, P.map_extrinsics(frames, False)):
        m.build_3D_map(RGBDImage(col, dep), intr, E)
    mesh = m.extract_mesh()
    scene = RC.RaycastingScene()
    scene.add_triangles(mesh)
    E = np.linalg.inv(frames[3][2])
    rays = RC.RaycastingScene.create_rays_pinhole(M.pinhole_matrix(P.MAP_K), E, P.MAP_W, P.MAP_H, pixel_center=0.0)
    out = scene.cast_rays(rays)
    assert scene.n_triangles == len(mesh.triangles) > 40000 and scene.n_kept > 0.99 * scene.n_triangles
    part = rays.reshape(-1, 6)[5::16].numpy()                                          # 192 rays against the statement on the same mesh
    ref = M.cast_rays(M.Scene((mesh.vertices, mesh.triangles)), part)
    assert_equals_statement({k: v.reshape((-1,) + tuple(v.shape[2:]))[5::16] for k, v in out.items()}, ref, "map mesh")
    t_hit = out["t_hit"].cpu().numpy()
    hit = np.isfinite(t_hit)
    cast = m.raycast(intr, E, depth_min=0.05, depth_max=1.0).depth.cpu().numpy().reshape(P.MAP_H, P.MAP_W)
    analytic = R.render(frames[3][2], P.MAP_K, P.MAP_H, P.MAP_W)[1]
    both = hit & (cast > 0)
    print("hits: mesh", hit.sum(), "tsdf ray cast", (cast > 0).sum(), "both", both.sum(), "mesh - ray cast max", np.abs(t_hit[both] - cast[both]).max(),
          "mesh - analytic max", np.abs(t_hit[both] - analytic[both]).max())
    assert both.sum() > 2900                                                         # (the oracle: 3 020 of 3 072 pixels)
    # Both bounds: the maximum measured on the CPU with oracle/tsdf_ref.py's volume and mesh run through the statement and
    # tests/_raycast_ref.py -- 2.52e-4 m against the TSDF ray cast, 2.02e-4 m against the analytic depth -- plus one voxel edge, 2 mm (the
    # device's mesh differs from the oracle's by rounding and by vertex order)
    assert np.abs(t_hit[both] - cast[both]).max() <= 2.52e-4 + P.MAP_VL
    assert np.abs(t_hit[both] - analytic[both]).max() <= 2.02e-4 + P.MAP_VL
