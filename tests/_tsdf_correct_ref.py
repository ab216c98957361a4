"""Numpy statement of TSDF de-integration (csrc/tsdf.hip tsdf_blend / tsdf_unblend) -- TEST INFRASTRUCTURE ONLY.

A subclass of the oracle's TSDFRef whose ``integrate`` / ``deintegrate`` restate the DEVICE's blend arithmetic -- the weight's rounded
reciprocal times fmaf(value, w0, +-x), the fused multiply-add emulated as an fp64 product and sum rounded once to fp32 -- and the
reset and skip rules of tsdf_unblend.  What a frame says about a voxel (the observation) is the oracle's, so this is neither a copy
of the kernel nor the oracle: the oracle stays the independent check of plain integration, this file states what taking a frame out
again must leave.  Nothing of it comes from Open3D or from the reference, neither of which has the operation.

Also here, shared by tests/test_map_correction_cpu.py and tests/test_map_correction_gpu.py: the small scene of tests/test_tsdf_gpu.py
(a copy), the seeded six-round correction experiment, and the gaps the statement measured for it (the GPU bars are 8 x those).
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from oracle.tsdf_ref import TSDFRef  # noqa: E402

H, W = 48, 64
K = (60.0, 60.0, 32.0, 24.0)
VL, TRUNC = 0.01, 0.04


def scene(seed):
    """tests/test_tsdf_gpu.py's scene(seed): depth fp32 [H, W] with holes, colour u8 [H, W, 3], extrinsic 4x4"""
    rng = np.random.default_rng(seed)
    v, u = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    depth = (0.5 + 0.05 * np.sin(u / 9.0 + seed) * np.cos(v / 7.0)).astype(np.float32)
    depth[rng.random((H, W)) < 0.03] = 0.0                                  # holes
    color = rng.integers(0, 256, size=(H, W, 3)).astype(np.uint8)
    a = 0.05 * seed
    pose = np.eye(4)
    pose[:3, :3] = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    pose[:3, 3] = (0.03 * seed, -0.02 * seed, 0.01 * seed)
    return depth, color, np.linalg.inv(pose)


# ---- the correction experiment --------------------------------------------------------------------------------------------------
N_FRAMES, N_ROUNDS, MOVED_PER_ROUND = 6, 6, 3
JITTER_T, JITTER_R = 0.01, 0.02            # metres, radians (scale of the normal draws)

# worst |correction - fresh| the statement measured after round r = 1..6 of this experiment at (res, stride) = (8, 4) with colours
# ((4, 8) measures the same or less); tests/test_map_correction_cpu.py prints them and holds them to these values, rounded up.
# tsdf, then colour (colours on 0..255)
STATEMENT_GAP_TSDF = (3.0e-7, 4.2e-7, 4.8e-7, 6.3e-7, 9.0e-7, 9.6e-7)      # measured 2.98e-7 4.17e-7 4.77e-7 6.26e-7 8.94e-7 9.54e-7
STATEMENT_GAP_COLOR = (6.2e-5, 9.2e-5, 9.2e-5, 1.4e-4, 1.6e-4, 1.9e-4)     # measured 6.10e-5 9.16e-5 9.16e-5 1.37e-4 1.53e-4 1.83e-4
BAR_FACTOR = 8.0                           # device bar = 8 x the statement's gap (DESIGN section 3.14's convention)


def jitter(rng):
    """a small rigid motion: rotation vector ~ N(0, JITTER_R) per axis, translation ~ N(0, JITTER_T) per axis"""
    w = rng.normal(size=3) * JITTER_R
    th = float(np.linalg.norm(w))
    Kx = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    R = np.eye(3) if th == 0.0 else np.eye(3) + np.sin(th) / th * Kx + (1 - np.cos(th)) / (th * th) * Kx @ Kx
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, rng.normal(size=3) * JITTER_T
    return T


def correction_rounds(seed=11):
    """the poses after each of the N_ROUNDS rounds: round r moves MOVED_PER_ROUND seeded frames by a seeded jitter.  Yields
    (round 1.., the frames moved, the list of all N_FRAMES extrinsics after the round)"""
    rng = np.random.default_rng(seed)
    poses = [scene(s)[2] for s in range(N_FRAMES)]
    for r in range(1, N_ROUNDS + 1):
        which = sorted(int(j) for j in rng.choice(N_FRAMES, size=MOVED_PER_ROUND, replace=False))
        poses = [p.copy() for p in poses]
        for j in which:
            poses[j] = jitter(rng) @ poses[j]
        yield r, which, poses


# ---- the statement ------------------------------------------------------------------------------------------------------------------
def _fmaf(a, b, c):
    """fmaf(a, b, c) on fp32 arrays: the product is exact in fp64, the sum is rounded to fp64 and then once more to fp32"""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


class TSDFCorrectRef(TSDFRef):
    """TSDFRef with the device's blend and its inverse.  ``misuse`` counts the voxel observations a deintegrate skipped because
    the voxel's weight was below 1 (the device raises counters[2] = 3 for them)."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.misuse = 0

    def _observe(self, key, depth, color, Kc, E):
        """what the frame says about the voxels of unit `key`, as TSDFRef.integrate states it: (ok, tsdf fp32, colour fp32 or None)"""
        fx, fy, cx, cy = Kc
        Hh, Ww = depth.shape
        r = self.res
        g = (np.arange(r) + 0.5) * self.vl
        o = np.array(key, dtype=np.float64) * self.L
        X, Y, Z = np.meshgrid(g + o[0], g + o[1], g + o[2], indexing="ij")
        qx = E[0, 0] * X + E[0, 1] * Y + E[0, 2] * Z + E[0, 3]
        qy = E[1, 0] * X + E[1, 1] * Y + E[1, 2] * Z + E[1, 3]
        qz = E[2, 0] * X + E[2, 1] * Y + E[2, 2] * Z + E[2, 3]
        ok = qz > 0
        qzs = np.where(ok, qz, 1.0)
        uf = qx * fx / qzs + cx + 0.5
        vf = qy * fy / qzs + cy + 0.5
        ok &= (uf >= 0.0001) & (uf < Ww - 0.0001) & (vf >= 0.0001) & (vf < Hh - 0.0001)
        ui = np.where(ok, uf, 0).astype(int)
        vi = np.where(ok, vf, 0).astype(int)
        d = depth[vi, ui]
        ok &= d > 0
        xx = ((ui - cx) / fx).astype(np.float32)
        yy = ((vi - cy) / fy).astype(np.float32)
        mult = np.sqrt(xx * xx + yy * yy + np.float32(1.0), dtype=np.float32)
        sdf = ((d.astype(np.float64) - qz) * mult.astype(np.float64)).astype(np.float32)
        ok &= sdf > -np.float32(self.trunc)
        t = np.minimum(np.float32(1.0), sdf * np.float32(1.0 / self.trunc))
        c = None if color is None else np.asarray(color)[vi, ui].astype(np.float32)
        return ok, t, c

    def integrate(self, depth, color, Kc, extrinsic):
        depth = np.asarray(depth, dtype=np.float32)
        E = np.asarray(extrinsic, dtype=np.float64)
        r = self.res
        for key in sorted(self.touched(depth, Kc, extrinsic)):
            vox = self.units.setdefault(key, np.zeros((r, r, r, 5), dtype=np.float32))
            ok, t, c = self._observe(key, depth, color, Kc, E)
            w0 = vox[..., 1].copy()
            w1 = w0 + np.float32(1.0)
            rw = np.float32(1.0) / w1
            vox[..., 0] = np.where(ok, _fmaf(vox[..., 0], w0, t) * rw, vox[..., 0])
            if c is not None:
                for k in range(3):
                    vox[..., 2 + k] = np.where(ok, _fmaf(vox[..., 2 + k], w0, c[..., k]) * rw, vox[..., 2 + k])
            vox[..., 1] = np.where(ok, w1, w0)

    def deintegrate(self, depth, color, Kc, extrinsic):
        """tsdf_unblend over the frame's units: weight < 1 -> skipped and counted; weight back to 0 -> five +0.0f; else the inverse blend"""
        depth = np.asarray(depth, dtype=np.float32)
        E = np.asarray(extrinsic, dtype=np.float64)
        for key in sorted(self.touched(depth, Kc, extrinsic)):
            vox = self.units.get(key)
            ok, t, c = self._observe(key, depth, color, Kc, E)
            if vox is None:                      # the unit was never opened: every observation of it is a misuse
                self.misuse += int(ok.sum())
                continue
            w0 = vox[..., 1].copy()
            self.misuse += int((ok & (w0 < 1)).sum())
            ok = ok & (w0 >= 1)
            w1 = w0 - np.float32(1.0)
            wipe = ok & (w1 == 0)
            go = ok & (w1 != 0)
            with np.errstate(divide="ignore", invalid="ignore"):
                rw = np.float32(1.0) / w1
                vox[..., 0] = np.where(go, _fmaf(vox[..., 0], w0, -t) * rw, vox[..., 0])
                if c is not None:
                    for k in range(3):
                        vox[..., 2 + k] = np.where(go, _fmaf(vox[..., 2 + k], w0, -c[..., k]) * rw, vox[..., 2 + k])
            vox[..., 1] = np.where(go, w1, w0)
            vox[wipe] = np.float32(0.0)


def compare_maps(units_corrected, units_fresh):
    """the properties a corrected map owes a fresh one (both: dict key -> fp32 [r, r, r, 5]).  Asserts the exact ones -- the fresh map's
    units are a subset, the extra units are all zero, weights are bit-equal, every weight-0 voxel is wholly zero -- and returns the
    worst |delta tsdf| and |delta colour|."""
    assert set(units_fresh) <= set(units_corrected), "a unit of the fresh map is missing from the corrected one"
    gap_t = gap_c = 0.0
    for key, got in units_corrected.items():
        want = units_fresh.get(key)
        if want is None:
            assert not got.view(np.uint32).any(), f"extra unit {key} is not all zero"
            continue
        assert np.array_equal(got[..., 1], want[..., 1]), f"weights of unit {key}"
        assert not got[got[..., 1] == 0].view(np.uint32).any(), f"a weight-0 voxel of unit {key} is not wholly zero"
        gap_t = max(gap_t, float(np.abs(got[..., 0] - want[..., 0]).max()))
        gap_c = max(gap_c, float(np.abs(got[..., 2:] - want[..., 2:]).max()))
    return gap_t, gap_c
