"""The triangle-mesh scene without a GPU: the numpy statement (tests/_mesh_scene_ref.py) on scenes whose answer is known in closed form --
a cube whose triangles lie in dyadic planes, an icosphere, a height field against the analytic renderer, two triangles of known area
ratio --, degenerate scenes and ties, the public interface (signatures, argument validation, the documents' caveats) and no CPU fallback."""
import inspect
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _mesh_scene_ref as M  # noqa: E402
import _pointcloud_ref as P  # noqa: E402
import _render as R  # noqa: E402

f32 = np.float32


def origin_rays(dirs):
    d = np.asarray(dirs).astype(f32)
    return np.concatenate([np.zeros_like(d), d], 1)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.fixture(scope="module")
def cube():
    v, t = M.cube()
    assert len(t) == 192
    return v, t, M.Scene((v, t))


# ---- rays ------------------------------------------------------------------------------------------------------------------------------------
def test_cube_no_ray_slips_through(cube):
    """from the centre to every vertex, to every edge midpoint and in 4 096 random directions: zero misses, although every ray of the first
    two kinds lies exactly in shared edges or vertices of the dyadic triangulation"""
    v, t, scene = cube
    mids = np.concatenate([(v[t[:, a]] + v[t[:, b]]) / 2 for a, b in ((0, 1), (1, 2), (2, 0))])
    dirs = np.concatenate([v, mids, np.random.default_rng(0).normal(size=(4096, 3))]).astype(f32)
    out = M.cast_rays(scene, origin_rays(dirs))
    assert np.isfinite(out["t_hit"]).all()
    assert (out["geometry_ids"] == 0).all() and (out["primitive_ids"] < 192).all()
    # the hit lies on the cube: max |o + t d| = 1, exactly for the lattice directions (one coordinate is +-1, t = 1)
    assert np.array_equal(out["t_hit"][:len(v) + len(mids)], np.ones(len(v) + len(mids), f32))
    reach = np.abs(dirs * out["t_hit"][:, None]).max(1)
    assert np.abs(reach - 1.0).max() < 4e-7
    # the uvs give the same point, and the normal is the face's
    c = M.corners(v, t)
    pid = out["primitive_ids"].astype(np.int64)
    u, w = out["primitive_uvs"][:, 0:1].astype(np.float64), out["primitive_uvs"][:, 1:2].astype(np.float64)
    p = (1 - u - w) * c[0][pid] + u * c[1][pid] + w * c[2][pid]
    assert np.abs(p - dirs.astype(np.float64) * out["t_hit"][:, None]).max() < 1e-6
    assert (u >= 0).all() and (w >= 0).all() and (u + w <= 1 + 1e-6).all()
    n = out["primitive_normals"]
    assert np.array_equal(np.abs(n).max(1), np.ones(len(n), f32)) and np.array_equal(np.abs(n).sum(1), np.ones(len(n), f32))


def test_cube_axis_rays_scale_with_the_direction(cube):
    _, _, scene = cube
    axes = np.concatenate([np.eye(3), -np.eye(3)]).astype(f32)
    for length in (1.0, 2.0 ** -10, 2.0 ** 10, 1e-3, 1e3):
        out = M.cast_rays(scene, origin_rays(axes * f32(length)))
        assert np.allclose(out["t_hit"] * f32(length), 1.0, rtol=3e-7, atol=0)
        if np.log2(length) == int(np.log2(length)):
            assert np.array_equal(out["t_hit"], np.full(6, 1.0 / length, f32))
    # from outside: the near face, two-sided; pointing away: a miss
    out = M.cast_rays(scene, np.array([[3, 0.25, 0.25, -1, 0, 0], [3, 0.25, 0.25, 1, 0, 0], [0.25, -5, 0.3, 0, 2, 0]], f32))
    assert np.array_equal(out["t_hit"], np.array([2.0, np.inf, 2.0], f32))
    assert out["primitive_ids"][1] == M.INVALID and out["geometry_ids"][1] == M.INVALID and not out["primitive_normals"][1].any()


def test_icosphere_no_ray_slips_through():
    v, t = M.icosphere(2)
    assert len(t) == 320
    scene = M.Scene((v, t))
    dirs = np.concatenate([v, np.random.default_rng(1).normal(size=(4096, 3))]).astype(f32)
    out = M.cast_rays(scene, origin_rays(dirs))
    assert np.isfinite(out["t_hit"]).all()
    assert np.abs(out["t_hit"][:len(v)] - 1.0).max() < 5e-7                 # a ray to a vertex hits at the vertex
    r = np.linalg.norm(dirs.astype(np.float64) * out["t_hit"][:, None], axis=1)
    assert r.max() < 1 + 1e-6 and r.min() > 0.97                           # inside the sphere, outside the inscribed one of the level-2 facets


def test_special_rays(cube):
    _, _, scene = cube
    rays = np.array([[0, 0, 0, 0, 0, 0], [0, 0, 0, np.nan, 0, 1], [np.inf, 0, 0, 1, 0, 0], [0, 0, 0, np.inf, 0, 0], [0, 0, 0, 0.0, -0.0, 1],
                     [0, 0, 0, -0.0, 0.0, -1], [1, 0.25, 0.25, 1, 0, 0], [1, 0.25, 0.25, -1, 0, 0], [0.5, 0.5, -2, 0, 0, 1]], f32)
    out = M.cast_rays(scene, rays)
    assert np.array_equal(bits(out["t_hit"]), bits(np.array([np.inf, np.inf, np.inf, np.inf, 1, 1, 0, 0, 1], f32)))       # (+0, never -0)
    assert (out["primitive_ids"][:4] == M.INVALID).all() and (out["primitive_ids"][4:] != M.INVALID).all()
    # [..., 6] shapes pass through
    out2 = M.cast_rays(scene, rays.reshape(3, 3, 6))
    assert out2["t_hit"].shape == (3, 3) and out2["primitive_normals"].shape == (3, 3, 3) and np.array_equal(bits(out2["t_hit"]).ravel(), bits(out["t_hit"]))


def test_ties_and_degenerate_scenes():
    v, t = M.grid_patch(np.linspace(-1, 1, 5), np.linspace(-1, 1, 5), lambda X, Y: np.ones_like(X))
    rays = origin_rays(np.concatenate([np.random.default_rng(2).uniform(-0.9, 0.9, (64, 2)), np.ones((64, 1))], 1))
    one = M.cast_rays(M.Scene((v, t)), rays)
    twice = M.cast_rays(M.Scene((v, np.concatenate([t, t]))), rays)                    # the patch twice in one geometry: the lower row
    assert np.array_equal(twice["primitive_ids"], one["primitive_ids"]) and np.array_equal(bits(twice["t_hit"]), bits(one["t_hit"]))
    two = M.cast_rays(M.Scene((v, t), (v, t)), rays)                                   # as two geometries: geometry 0
    assert (two["geometry_ids"] == 0).all() and np.array_equal(two["primitive_ids"], one["primitive_ids"])
    far = M.cast_rays(M.Scene((v + f32(1), t), (v, t)), rays)                          # the nearer geometry wins whatever its id
    assert (far["geometry_ids"] == 1).all() and np.array_equal(far["primitive_ids"], one["primitive_ids"])
    q = np.array([[0.1, 0.2, 3.0], [np.nan, 0, 0]], f32)
    assert np.array_equal(M.closest_points(M.Scene((v, t), (v, t)), q)["geometry_ids"], np.array([0, M.INVALID], np.uint32))
    # an empty scene
    empty = M.Scene()
    out = M.cast_rays(empty, rays)
    assert np.isinf(out["t_hit"]).all() and (out["primitive_ids"] == M.INVALID).all()
    c = M.closest_points(empty, q)
    assert np.isinf(c["distance"][0]) and np.isnan(c["distance"][1]) and (c["primitive_ids"] == M.INVALID).all() and np.isnan(c["points"]).all()
    # a zero-area triangle and one with a NaN vertex among valid ones are never reported, and rows keep their numbers
    vv = np.concatenate([v, [[np.nan, 0, 1], [0, 0, 0.5], [0.5, 0.5, 0.5], [1, 1, 0.5]]]).astype(f32)
    n = len(v)
    tt = np.concatenate([[[0, 1, n], [n + 1, n + 2, n + 3], [3, 3, 3]], t]).astype(np.int32)
    scene = M.Scene((vv, tt))
    assert not scene.kept[:3].any() and scene.kept[3:].all()
    out = M.cast_rays(scene, rays)
    assert np.array_equal(out["primitive_ids"], one["primitive_ids"] + 3) and np.array_equal(bits(out["t_hit"]), bits(one["t_hit"]))
    c = M.closest_points(scene, np.array([[0.25, 0.25, 0.5]], f32))                     # on the collinear triangle: the patch is 0.5 away
    assert c["distance"][0] == f32(0.5) and c["primitive_ids"][0] >= 3
    # a single triangle
    single = M.Scene((np.array([[0, 0, 1], [1, 0, 1], [0, 1, 1]], f32), np.array([[0, 1, 2]], np.int32)))
    out = M.cast_rays(single, origin_rays([[0.25, 0.25, 1], [1, 1, 1], [0, 0, 1], [0.5, 0.5, 1]]))
    assert np.array_equal(out["t_hit"], np.array([1, np.inf, 1, 1], f32)) and np.array_equal(out["primitive_uvs"][0], np.array([0.25, 0.25], f32))


def test_pinhole_depth_against_the_analytic_renderer():
    """t_hit of create_rays_pinhole's rays IS the z-depth: the 2 mm height-field mesh against _render.render at pixel_center = 0"""
    v, t = M.height_field()
    assert len(t) == 5400
    scene = M.Scene((v, t))
    worst = 0.0
    for i in (2, 5):
        pose = P.map_frames()[i][2]
        rays = M.create_rays_pinhole(M.pinhole_matrix(P.MAP_K), np.linalg.inv(pose), P.MAP_W, P.MAP_H, pixel_center=0.0)
        assert rays.shape == (P.MAP_H, P.MAP_W, 6) and rays.dtype == f32
        assert np.abs(rays[..., :3] - pose[:3, 3]).max() < 1e-8 and np.abs(rays[..., 3:] @ pose[:3, 2].astype(f32) - 1).max() < 1e-6
        out = M.cast_rays(scene, rays)
        hit = np.isfinite(out["t_hit"])
        assert hit.sum() > 300
        worst = max(worst, float(np.abs(out["t_hit"][hit] - R.render(pose, P.MAP_K, P.MAP_H, P.MAP_W)[1][hit]).max()))
    # the tessellation error, about max |g''| pitch^2 / 8: measured 1.67e-6 m (frame 2), 1.61e-6 m (frame 5); the bound is twice the maximum
    assert worst <= 2 * 1.67e-6, worst
    half = M.create_rays_pinhole(M.pinhole_matrix(P.MAP_K), np.eye(4), 4, 3)           # Open3D's convention: the centre of pixel (0, 0)
    assert np.array_equal(half[0, 0], np.array([0, 0, 0, (0.5 - 32) / 60, (0.5 - 24) / 60, 1], np.float64).astype(f32))


# ---- closest points --------------------------------------------------------------------------------------------------------------------------
def test_cube_distances_are_exact(cube):
    v, _, scene = cube
    q = np.array([[2, 0.25, 0.25], [0.5, -3, 0.5], [2, 2, 2], [-1.5, 0.375, 3], [0, 0, 0], [0.25, 0.5, 0.75], [1, 1, 1], [0.5, 1, 0.25]], f32)
    c = M.closest_points(scene, q)
    assert np.array_equal(c["d2"], np.array([1, 4, 3, 4.25, 1, 0.0625, 0, 0], f32))
    assert np.array_equal(c["distance"], np.sqrt(np.array([1, 4, 3, 4.25, 1, 0.0625, 0, 0], f32)))
    assert np.array_equal(c["points"][:4], np.array([[1, 0.25, 0.25], [0.5, -1, 0.5], [1, 1, 1], [-1, 0.375, 1]], f32))
    on = M.closest_points(scene, v)                                                     # points exactly on vertices
    assert not on["d2"].any() and np.array_equal(on["points"], v)
    md = M.closest_points(scene, q, max_distance=1.0)
    assert np.array_equal(np.isinf(md["distance"]), np.array([0, 1, 1, 1, 0, 0, 0, 0], bool)) and np.isnan(md["points"][1]).all()


def test_closest_points_against_fp64():
    v, t = M.height_field()
    scene = M.Scene((v, t))
    src = P.base_source()[::8]
    q = np.concatenate([src, src + f32(0.5), v[::97], ((v[t[::301, 0]] + v[t[::301, 1]]) / 2).astype(f32)])
    c = M.closest_points(scene, q)
    a, b, cc = (x.astype(np.float64) for x in (scene.v0, scene.v1, scene.v2))
    pid = c["primitive_ids"].astype(np.int64)
    u, w = c["primitive_uvs"][:, 0:1].astype(np.float64), c["primitive_uvs"][:, 1:2].astype(np.float64)
    assert (u > -1e-6).all() and (w > -1e-6).all() and (u + w < 1 + 1e-6).all()
    p = (1 - u - w) * a[pid] + u * b[pid] + w * cc[pid]
    assert np.abs(p - c["points"]).max() < 2e-7                                          # the uvs give the point
    assert np.abs(np.linalg.norm(q - c["points"].astype(np.float64), axis=1) - c["distance"]).max() < 2e-7
    # no point of a fine sampling of the surface is closer than the reported distance (beyond the sampling's own pitch)
    k = np.linspace(0, 1, 6)
    bary = np.array([(1 - i - j, i, j) for i in k for j in k if i + j <= 1 + 1e-12])
    S = (bary[:, 0, None, None] * a + bary[:, 1, None, None] * b + bary[:, 2, None, None] * cc).reshape(-1, 3)
    for i in range(0, len(q), 37):
        d = np.linalg.norm(S - q[i].astype(np.float64), axis=1).min()
        assert c["distance"][i] <= d + 1e-7 and d <= c["distance"][i] + 0.002 * 0.5
    nv = len(v[::97])
    assert not c["distance"][len(src) * 2:len(src) * 2 + nv].any()                        # on vertices: exactly 0
    # an edge's midpoint is rounded to fp32: off the edge by at most half an ulp of 0.35 per coordinate, sqrt(3) 1.5e-8
    assert (c["distance"][len(src) * 2 + nv:] < 3e-8).all()


# ---- sampling --------------------------------------------------------------------------------------------------------------------------------
def test_sampling_statistics_and_batches():
    v = np.array([[0, 0, 0], [3, 0, 0], [0, 2, 0], [5, 0, 0], [6, 0, 0], [5, 2, 0]], f32)
    t = np.array([[0, 1, 2], [3, 4, 5]], np.int32)                                        # areas 3 : 1
    col = np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1]] * 2, f32)
    n = 2 ** 16
    pts, c, nrm, idx = M.sample_mesh(v, t, n, seed=0, vertex_colors=col)
    share = float((idx == 0).mean())
    assert abs(share - 0.75) <= 5 * np.sqrt(0.75 * 0.25 / n), share                       # 0.74792 with seed 0 (0.0083 allowed)
    assert (c >= 0).all() and np.abs(c.sum(1) - 1).max() < 3e-7                           # the colours ARE the barycentric weights here
    inside0 = (pts[idx == 0, 0] / 3 + pts[idx == 0, 1] / 2 <= 1 + 1e-6) & (pts[idx == 0] >= 0).all(1)
    inside1 = (pts[idx == 1, 0] >= 5) & (pts[idx == 1, 1] >= 0) & ((pts[idx == 1, 0] - 5) + pts[idx == 1, 1] / 2 <= 1 + 1e-6)
    assert inside0.all() and inside1.all() and not pts[:, 2].any()
    assert np.array_equal(nrm, np.tile(np.array([0, 0, 1], f32), (n, 1)))
    # uniform inside a triangle: the centroid
    assert np.abs(pts[idx == 0].mean(0) - [1, 2 / 3, 0]).max() < 0.01
    # every sample reproduces from (seed, i) alone, for any batch split
    for first, m in ((0, 1), (1, 63), (64, 65), (129, 4099), (n - 5, 5)):
        b = M.sample_mesh(v, t, m, seed=0, vertex_colors=col, first=first)
        assert np.array_equal(bits(b[0]), bits(pts[first:first + m])) and np.array_equal(b[3], idx[first:first + m])
        assert np.array_equal(bits(b[1]), bits(c[first:first + m]))
    other = M.sample_mesh(v, t, 1024, seed=1)
    assert other[1] is None and not np.array_equal(other[3], idx[:1024])
    # a zero-area and a NaN triangle take no sample; a mesh of only such triangles gives an empty cloud
    v2 = np.concatenate([v, [[np.nan, 0, 0]]]).astype(f32)
    t2 = np.array([[0, 0, 1], [0, 1, 6], [3, 4, 5], [0, 1, 2]], np.int32)
    assert set(M.sample_mesh(v2, t2, 4096)[3]) == {2, 3}
    e = M.sample_mesh(v2, t2[:2], 16, vertex_colors=np.zeros((7, 3), f32))
    assert e[0].shape == (0, 3) and e[1].shape == (0, 3) and e[2].shape == (0, 3) and e[3].shape == (0,) and e[3].dtype == np.int32


def test_the_hash_is_splitmix64():
    """mix64 is the output function of splitmix64: its first outputs for the state 0 are published with the generator"""
    z = (np.arange(1, 4, dtype=np.uint64) * M.GOLDEN)
    assert [int(x) for x in M.mix64(z)] == [0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4, 0x06C45D188009454F]
    assert int(M.mulhi64(np.array([2 ** 63], np.uint64), np.uint64(10))[0]) == 5


# ---- the grid: the statement's two walks equal its brute force, bit for bit, at three cell sizes ------------------------------------------
def same(a, b):
    for k in b:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        assert x.shape == y.shape and ((x == y) | ((x != x) & (y != y))).all(), k


def grid_rays(v, t):
    """the special rays of the GPU tests (from inside, from the boundary, from 10^3 extents away, along lattice planes and edges, +-0
    components, zero / NaN / inf rays), thinned"""
    import test_mesh_scene_gpu as G
    rays, odd = G.special_rays(v, t, v.min(0), v.max(0))
    return np.concatenate([rays[::6], odd]), len(rays[384:576:6])          # (rays 384 .. 575 start far away: every sixth of them)


@pytest.mark.parametrize("which", ["cube", "icosphere", "field", "ties", "degenerate"])
def test_grid_equals_brute_force(which):
    rng = np.random.default_rng(5)
    if which == "cube":
        geoms = [M.cube()]
    elif which == "icosphere":
        geoms = [M.icosphere(2)]
    elif which == "field":
        geoms = [M.height_field()]
    else:
        v, t = M.grid_patch(np.linspace(-1, 1, 5), np.linspace(-1, 1, 5), lambda X, Y: np.ones_like(X))
        if which == "ties":
            geoms = [(v, np.concatenate([t, t])), (v, t)]
        else:                                       # NaN and zero-area rows, and a floor triangle far larger than the patch
            vv = np.concatenate([v, [[np.nan, 0, 1], [0, 0, 0.5], [0.5, 0.5, 0.5], [1, 1, 0.5]]]).astype(f32)
            tt = np.concatenate([[[0, 1, 25], [26, 27, 28], [3, 3, 3]], t]).astype(np.int32)
            geoms = [(vv, tt), (np.array([[-50, -50, 0.5], [50, -50, 0.5], [0, 80, 0.5]], f32), np.array([[0, 1, 2]], np.int32))]
    scene = M.Scene(*geoms)
    v, t = geoms[0]
    v = v[np.isfinite(v).all(1)]
    rays, n_far = grid_rays(v, t)
    centre = (v.min(0) + v.max(0)) / 2
    d = rng.normal(size=(48, 3)).astype(f32)
    rays = np.concatenate([rays, np.concatenate([np.tile(centre, (48, 1)), d], 1).astype(f32)])
    q = np.concatenate([rng.uniform(v.min(0) - 0.2, v.max(0) + 0.2, (40, 3)), v[::max(len(v) // 20, 1)], (v[:8] + 40 * (v.max(0) - v.min(0)).max()),
                        [[np.nan, 0, 0]]]).astype(f32)
    ref, cref = M.cast_rays(scene, rays), M.closest_points(scene, q)
    cref_md = M.closest_points(scene, q, max_distance=0.05)
    base = M.Grid(scene)
    assert base.n_refs <= M.max_refs(len(scene.kept)) and int(np.prod(base.dims)) <= M.MAX_CELLS
    for mult in (1.0, 0.5, 3.0):
        try:
            grid = base if mult == 1.0 else M.Grid(scene, base.h * f32(mult))
        except ValueError:                          # (half the default can break the reference cap: the floor triangle spans every cell)
            assert which == "degenerate" and mult == 0.5
            continue
        st = {}
        same(M.cast_rays_grid(grid, rays, st), ref)
        if which != "degenerate":                   # (there the floor makes the box so large that nothing starts far from it)
            assert st["fallback"] == n_far
        same(M.closest_points_grid(grid, q, stats_out=st), cref)
        same(M.closest_points_grid(grid, q, max_distance=0.05), cref_md)
    if which == "degenerate":
        with pytest.raises(ValueError):             # more than 2^24 cells
            M.Grid(scene, 1e-4)


def slabs(n=2048):
    """n triangles that each span the whole box in x and y, stacked in z: about n cells by default, and every triangle in a whole layer"""
    z = np.linspace(0, 1, n)
    v = np.stack([np.tile([0.0, 1.0, 0.0], n), np.tile([0.0, 0.0, 1.0], n), np.repeat(z, 3)], 1).astype(f32)
    return v, np.arange(3 * n, dtype=np.int32).reshape(n, 3)


def test_reference_cap_grows_the_default_cell():
    v, t = slabs()
    scene = M.Scene((v, t))
    grid = M.Grid(scene)
    first = f32(_P_default(scene))
    refs_at = lambda h: int(sum(len(x) for x in M.Grid(scene, h).lists.values()))
    assert grid.h > first and grid.n_refs <= M.max_refs(len(t)) == 2 ** 16
    with pytest.raises(ValueError):                 # the first guess itself breaks the cap, so as an explicit size it is refused
        M.Grid(scene, first)
    assert refs_at(grid.h) == grid.n_refs
    rays = np.concatenate([np.tile([0.3, 0.3, -1.0], (16, 1)), np.random.default_rng(6).normal(size=(16, 3)) * 0.1 + [0, 0, 1]], 1).astype(f32)
    same(M.cast_rays_grid(grid, rays), M.cast_rays(scene, rays))


def _P_default(scene):
    k = scene.kept
    pts = np.concatenate([scene.v0[k], scene.v1[k], scene.v2[k]])
    return P.default_cell_size(pts.min(0), pts.max(0), int(k.sum()))


# ---- the public interface ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    import bodyslam_amd.evaluation as EV
    import bodyslam_amd.pointcloud as PC
    import bodyslam_amd.raycasting as RC
    import bodyslam_amd.tsdf as TS
    return RC, PC, EV, TS


def test_public_signatures(built):
    RC, PC, EV, TS = built

    def params(fn):
        return [(p.name, p.default) for p in inspect.signature(fn).parameters.values()]
    E = inspect.Parameter.empty
    assert params(RC.RaycastingScene.__init__) == [("self", E), ("device", 0), ("cell_size", None)]
    assert params(RC.RaycastingScene.cast_rays)[2:] == [("method", "grid")] and RC.METHODS == ("grid", "brute")
    assert params(RC.RaycastingScene.add_triangles) == [("self", E), ("vertices", E), ("triangles", None)]
    assert params(RC.RaycastingScene.cast_rays)[:2] == [("self", E), ("rays", E)]
    assert params(RC.RaycastingScene.create_rays_pinhole) == [("intrinsic_matrix", E), ("extrinsic_matrix", E), ("width_px", E), ("height_px", E),
                                                              ("pixel_center", 0.5)]
    assert isinstance(inspect.getattr_static(RC.RaycastingScene, "create_rays_pinhole"), staticmethod)
    assert params(RC.RaycastingScene.compute_closest_points)[:3] == [("self", E), ("query", E), ("max_distance", None)]
    assert params(RC.RaycastingScene.compute_distance)[:3] == [("self", E), ("query", E), ("max_distance", None)]
    assert params(TS.TriangleMesh.sample_points_uniformly) == [("self", E), ("number_of_points", E), ("seed", 0), ("host", None)]
    assert params(PC.sample_mesh)[:3] == [("vertices", E), ("triangles", E), ("number_of_points", E)]
    assert dict(params(PC.sample_mesh)[3:]) == dict(vertex_colors=None, seed=0, first=0, device=0)
    assert params(EV.evaluate_reconstruction_surface) == params(EV.evaluate_reconstruction) + [("align", None), ("icp", None), ("gt_mesh", "surface"),
                                                                                                ("n_gt_samples", None)]
    assert [f.name for f in __import__("dataclasses").fields(TS.TriangleMesh)] == ["vertices", "vertex_colors", "triangles"]
    assert RC.INVALID_ID == M.INVALID
    for doc in (RC.__doc__, PC.sample_mesh.__doc__):
        assert "unpinned" in doc.lower()
    assert "Not built" in RC.__doc__ and "Poisson-disk" in PC.__doc__.split("Not built")[1]
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hip = open(os.path.join(root, "bodyslam_amd", "csrc", "mesh_scene.hip")).read()
    assert "UNPINNED" in hip.split("#include")[0] and "tests/_mesh_scene_ref.py" in hip.split("#include")[0]
    design = open(os.path.join(root, "DESIGN.md")).read()
    assert "3.20" in design and "UNPINNED" in design.split("3.20")[1]


def test_pinhole_rays_equal_the_statement(built):
    RC = built[0]
    pose = P.map_frames()[3][2]
    K, E = M.pinhole_matrix(P.MAP_K), np.linalg.inv(pose)
    for pc in (0.5, 0.0):
        mine = RC.RaycastingScene.create_rays_pinhole(K, E, P.MAP_W, P.MAP_H, pixel_center=pc)
        assert isinstance(mine, torch.Tensor) and mine.dtype == torch.float32 and tuple(mine.shape) == (P.MAP_H, P.MAP_W, 6)
        assert np.array_equal(bits(mine.numpy()), bits(M.create_rays_pinhole(K, E, P.MAP_W, P.MAP_H, pixel_center=pc)))
    assert np.array_equal(bits(RC.RaycastingScene.create_rays_pinhole(torch.from_numpy(K), torch.from_numpy(E), 5, 4).numpy()),
                          bits(M.create_rays_pinhole(K, E, 5, 4)))
    for bad in (dict(intrinsic_matrix=np.eye(4)), dict(extrinsic_matrix=np.eye(3)), dict(width_px=0), dict(height_px=2.5), dict(width_px=True),
                dict(pixel_center=np.nan), dict(pixel_center="0"), dict(intrinsic_matrix=np.diag([0.0, 1, 1])),
                dict(extrinsic_matrix=np.full((4, 4), np.nan))):
        kw = dict(intrinsic_matrix=K, extrinsic_matrix=E, width_px=4, height_px=3)
        kw.update(bad)
        with pytest.raises(ValueError):
            RC.RaycastingScene.create_rays_pinhole(**kw)


def test_argument_validation(built):
    RC, PC, EV, TS = built
    v, t = M.cube()
    mesh = TS.TriangleMesh(v, np.zeros_like(v), t)
    assert RC.as_triangles(mesh)[1].shape == (192, 3) and RC.as_triangles(v.astype(np.float64), torch.from_numpy(t).long())[0].dtype == torch.float64
    for bad_v, bad_t in ((v[:, :2], t), (v.astype(np.int32), t), (v, t.astype(f32)), (v, t[:, :2]), (v, None), (None, t), (mesh, t), (v, t.tolist()),
                         (v, torch.from_numpy(t).bool()), (np.zeros((0, 3), f32), t)):
        with pytest.raises(ValueError):
            RC.as_triangles(bad_v, bad_t)
        with pytest.raises(ValueError):
            PC.sample_mesh(bad_v, bad_t, 8)
    for bad in (np.array([[0, 1, 150]]), np.array([[0, -1, 2]]), torch.tensor([[0, 1, 2 ** 40]])):
        with pytest.raises(ValueError):
            RC.check_indices(RC.as_triangles(v, bad)[1], len(v))
    RC.check_indices(RC.as_triangles(v, t)[1], len(v))
    for n in (0, -1, 2.5, True, "8", 2 ** 31):
        with pytest.raises(ValueError):
            PC.sample_mesh(v, t, n)
    for kw in (dict(seed=-1), dict(seed=2 ** 64), dict(seed=0.5), dict(first=-1), dict(vertex_colors=np.zeros((3, 3), f32)),
               dict(vertex_colors=np.zeros((150, 3), np.int32))):
        with pytest.raises(ValueError):
            PC.sample_mesh(v, t, 8, **kw)
    with pytest.raises(ValueError):
        PC.sample_mesh(np.zeros((3, 3), f32), np.zeros((2 ** 22 + 1, 3), np.int32), 8)
    for m in ("dda", "bvh", None):
        with pytest.raises(ValueError):
            RC._check_method(m)
    for bad in (np.zeros((4, 5), f32), np.zeros(6, np.int32), [[0.0] * 6], torch.zeros(2, 6, dtype=torch.float16)):
        with pytest.raises(ValueError):
            RC._as_rows(bad, 6, "rays")
    assert RC._as_rows(np.zeros((2, 3, 6)), 6, "rays").shape == (2, 3, 6)
    for dev in (-1, 0.5, True, "0"):
        with pytest.raises(ValueError):
            RC.RaycastingScene(device=dev)
    for cell in (0.0, -1.0, np.nan, np.inf, "1", True):
        with pytest.raises(ValueError):
            RC.RaycastingScene(cell_size=cell)
    pad, limit = RC.grid_padding(v.min(0), v.max(0))
    grid = M.Grid(M.Scene((v, t)))
    assert f32(pad) == grid.pad and f32(limit) == grid.o_limit and RC.max_references(192) == M.max_refs(192) == 2 ** 16
    # the evaluation: a surface needs a mesh, and the rest is checked before the GPU is touched
    pred = P.base_source()
    for kw in (dict(gt=v), dict(gt=TS.PointCloud(v, v)), dict(gt_mesh="faces"), dict(n_gt_samples=0), dict(n_gt_samples=1.5),
               dict(gt_mesh="vertices", n_gt_samples=8), dict(thresholds=(1,) * 9), dict(max_distance=-1.0), dict(align="icp"),
               dict(gt=TS.TriangleMesh(v, v, t[:0])), dict(icp=dict(max_correspondence_distance=0.01))):
        args = dict(pred=pred, gt=mesh)
        args.update(kw)
        with pytest.raises(ValueError):
            EV.evaluate_reconstruction_surface(**args)


def test_no_cpu_fallback(built):
    RC, PC, EV, TS = built
    if torch.cuda.is_available():
        return                                     # (tests/test_mesh_scene_gpu.py runs the same entry points there)
    from bodyslam_amd._lib import BodySlamHipError
    v, t = M.cube()
    mesh = TS.TriangleMesh(v, np.zeros_like(v), t)
    with pytest.raises(BodySlamHipError):
        RC.RaycastingScene()
    with pytest.raises(BodySlamHipError):
        PC.sample_mesh(v, t, 8)
    with pytest.raises(BodySlamHipError):
        mesh.sample_points_uniformly(8)
    with pytest.raises(BodySlamHipError):
        EV.evaluate_reconstruction_surface(P.base_source(), mesh)
    with pytest.raises(BodySlamHipError):
        EV.evaluate_reconstruction_surface(P.base_source(), mesh, gt_mesh="vertices")
