"""The numpy restatement of the TSDF ray cast (tests/_raycast_ref.py) against analytic truth: the yardstick of
tests/test_raycast_gpu.py is itself checked here, without a GPU.  The map is oracle.tsdf_ref.TSDFRef fed with four renderings of
tests/_render.py's height field; a ray cast of it must give back the renderer's own depth to half a voxel."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _raycast_ref as RC      # noqa: E402
import _render as R            # noqa: E402

H, W = RC.TOY_HW
K = RC.TOY_K


def build_ref(vl, trunc):
    from oracle.tsdf_ref import TSDFRef
    ref = TSDFRef(vl, trunc, res=8, stride=4)
    for P in RC.toy_poses():
        col, d = R.render(P, K, H, W)
        ref.integrate(d, col, K, np.linalg.inv(P))
    return ref


@pytest.fixture(scope="module", params=RC.TOY_MAPS, ids=lambda p: f"vl{p[0]}")
def toy(request):
    vl, trunc = request.param
    return vl, build_ref(vl, trunc)


def test_restatement_meets_analytic_depth_and_normals(toy):
    vl, ref = toy
    inner = np.zeros((H, W), bool)
    inner[4:-4, 4:-4] = True
    for name, P in zip(("seen0", "seen3", "unseen"), RC.toy_views()):
        got = RC.raycast(ref, K, np.linalg.inv(P), H, W, RC.DEPTH_MIN, RC.DEPTH_MAX, steps=True)
        _, truth = R.render(P, K, H, W)
        hit = got["depth"] > 0
        assert hit[inner].all(), f"{name}: {np.count_nonzero(~hit & inner)} interior pixels without a hit"
        err = np.abs(got["depth"] - truth)[hit] / vl
        print(f"vl {vl} {name}: hit share {hit.mean():.3f}, error in voxels median {np.median(err):.3f} max {err.max():.3f}, "
              f"steps mean {got['steps'].mean():.1f} max {got['steps'].max()}")
        assert err.max() <= 0.5, f"{name}: depth error {err.max():.3f} voxels"
        # normals at the interior hits: towards the camera, and along the height field's own normal line
        vtx = got["vertex"][hit & inner]
        nrm = np.array([ref.normal_at(p) for p in vtx])
        v, u = np.nonzero(hit & inner)
        d = np.stack([(u - K[2]) / K[0], (v - K[3]) / K[1], np.ones(len(u))], -1) @ P[:3, :3].T
        assert (np.sum(nrm * d, -1) < 0).all(), f"{name}: a normal faces away from the camera"
        an = RC.analytic_normal(vtx[:, 0], vtx[:, 1])
        ang = np.degrees(np.arccos(np.clip(np.abs(np.sum(nrm * an, -1)), 0.0, 1.0)))
        print(f"vl {vl} {name}: normal angle to the analytic line median {np.median(ang):.2f} max {ang.max():.2f} degrees")
        assert ang.max() <= 10.0, f"{name}: normal {ang.max():.1f} degrees off the analytic normal line"


def test_restatement_sees_nothing_where_nothing_is(toy):
    vl, ref = toy
    P = RC.toy_views()[0]
    back = P.copy()
    back[:3, :3] = P[:3, :3] @ np.diag([-1.0, 1.0, -1.0])                   # the same camera turned 180 degrees about its y axis
    got = RC.raycast(ref, K, np.linalg.inv(back), H, W, RC.DEPTH_MIN, RC.DEPTH_MAX, color=True)
    assert not got["depth"].any() and not got["vertex"].any() and not got["color"].any()
    # the surface lies at ~0.3 m: a ray cast that stops at 0.2 m must not find it
    got = RC.raycast(ref, K, np.linalg.inv(P), H, W, RC.DEPTH_MIN, 0.2)
    assert not got["depth"].any()


def test_restatement_on_an_empty_map():
    from oracle.tsdf_ref import TSDFRef
    ref = TSDFRef(0.01, 0.04, res=8, stride=4)
    got = RC.raycast(ref, K, np.eye(4), H, W, RC.DEPTH_MIN, RC.DEPTH_MAX, normal=True, color=True)
    assert all(not v.any() for v in got.values())


def test_restatement_colour_is_the_textures(toy):
    """colour of a seen view against the renderer's own u8 image: a trilinear mean of per-voxel running means of a texture with
    ~1 cm features cannot be exact, but it is the texture (mean absolute difference well under the texture's own contrast)"""
    vl, ref = toy
    P = RC.toy_views()[0]
    pix = np.stack(np.meshgrid(np.arange(8, H - 8, 4), np.arange(8, W - 8, 4), indexing="ij"), -1).reshape(-1, 2)
    got = RC.raycast(ref, K, np.linalg.inv(P), H, W, RC.DEPTH_MIN, RC.DEPTH_MAX, pixels=pix, color=True)
    col, _ = R.render(P, K, H, W)
    want = col[pix[:, 0], pix[:, 1]].astype(np.float64)
    diff = np.abs(got["color"].astype(np.float64) - want).mean()
    contrast = np.abs(want - want.mean(0)).mean()
    print(f"vl {vl}: colour mean |diff| {diff:.1f} of 255, texture contrast {contrast:.1f}")
    assert (got["depth"] > 0).all() and diff < 0.5 * contrast
