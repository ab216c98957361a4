"""Numpy statement of the voxel down-sampling (csrc/voxel.hip, bodyslam_amd/pointcloud.py) -- TEST INFRASTRUCTURE ONLY,
independent of the product code.

The role is Open3D's ``PointCloud.voxel_down_sample(voxel_size)`` -- the reference calls it at 3DM/mapping_module.py:72,156,187 with 0.005,
0.009 and 0.05 -- and, for the three index arrays, ``voxel_down_sample_and_trace``.  Open3D is not available: **parity unpinned**; the text
below restates the documented meaning (a regular grid of cubes of edge voxel_size, one output point per occupied cube, its position,
colour and normal the mean over the cube's points) and is the contract.  The reference only calls the function: there is nothing of
its own to pin.  Everything is exact in int64 and independent of the order of the points, except the row order, which is defined by it.

input     points are rounded to float32 once; a point with a non-finite coordinate belongs to no voxel, and nothing else of it is looked at
bounds    lo, hi: the float32 bounds of the finite points (`_pointcloud_ref.bounds`)
origin    o = float64(lo) - 0.5 h per axis, h the Python float as given, in float64
voxel     v = floor((float64(p) - o) / h) per axis in float64, one subtraction and one division; every component must be < 2^21, which is
          decided from hi alone (v is monotone in p): otherwise ValueError("voxel_size ... too small")
key       (vz << 42) | (vy << 21) | vx
rows      in order of first appearance: row r is the voxel whose lowest point index is the r-th smallest
position  ext = max over the axes of float64(hi) - o, ext = f 2^e with 0.5 <= f < 1 (frexp), s = 32 - e;
          Q = rint(ldexp(float64(p) - o, s)) as int64, 0 <= Q <= 2^32; per voxel S = sum Q, exact, below 2^63 for any count below 2^31;
          the result is float32(o + ldexp(float64(S) / float64(count), -s))
single    a voxel with exactly one point returns that point's bits -- its position, and its colour and normal too (unit_normals excepted:
          that always scales the mean).  A thinning does not change what it did not merge
colours, normals   when given, float32 [n, 3] (float64 is rounded once): Q = rint(float64(a) 2^30); every component of a point that belongs
          to a voxel must be finite with |a| <= 2, else ValueError; the result is float32(ldexp(float64(S) / float64(count), -30)), the
          plain mean.  unit_normals: the three means d in float64, len = sqrt((d0 d0 + d1 d1) + d2 d2), the result float32(d / len), zero
          when len is not positive
traced    counts int32 [m], first_index int32 [m] (the voxel's lowest point index), row_of_point int32 [n] (-1 for a non-finite point): the
          role of voxel_down_sample_and_trace in tensor form.  Open3D's own trace (an [m, 8] matrix of point indices by octant of the
          cube, and per-voxel index lists) is NOT restated.
no finite point   m = 0: empty [0, 3] arrays

Error bound (derived): against the float64 mean of the rounded points, a coordinate is off by at most 2^-(s+1) (every Q is within half a
unit of 2^-s, and so is their mean) plus half a float32 ulp of the result, before the rounding noise of the few float64 operations;
2^-(s+1) < ext 2^-32.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _pointcloud_ref as P  # noqa: E402

f32, f64 = np.float32, np.float64
AXIS_BITS = 21
ATTR_SHIFT = 30


def geometry(points, h):
    """-> (finite mask [n], o float64 [3], s) or (mask, None, None) without a finite point; ValueError when h needs 2^21 voxels on an axis"""
    pts = np.asarray(points).astype(f32)
    ok = np.isfinite(pts).all(1)
    if not ok.any():
        return ok, None, None
    lo, hi = P.bounds(pts)
    h = float(h)
    o = lo.astype(f64) - 0.5 * h
    ext = hi.astype(f64) - o
    with np.errstate(over="ignore", invalid="ignore"):
        top = np.floor(ext / h)
    if not (top < 2.0 ** AXIS_BITS).all():
        raise ValueError(f"voxel_size {h!r} too small: {top.max():.0f} voxels along an axis, at most 2^{AXIS_BITS}")
    _, e = np.frexp(ext.max())
    return ok, o, 32 - int(e)


def voxel_down_sample(points, h, colors=None, normals=None, unit_normals=False):
    """-> dict: points float32 [m, 3], colors / normals float32 [m, 3] or None, counts int32 [m], first_index int32 [m],
    row_of_point int32 [n], and for the tests origin float64 [3] and shift"""
    pts = np.asarray(points).astype(f32)
    n = len(pts)
    ok, o, s = geometry(pts, h)
    attrs = {}
    for name, a in (("colors", colors), ("normals", normals)):
        if a is not None:
            a = np.asarray(a).astype(f32)
            assert a.shape == pts.shape
            with np.errstate(invalid="ignore"):
                if not (np.abs(a[ok]) <= 2.0).all():                             # (false for NaN)
                    raise ValueError(f"{name}: every component must be finite with |a| <= 2")
            attrs[name] = a
    row_of_point = np.full(n, -1, np.int32)
    empty = np.zeros((0, 3), f32)
    if o is None:
        return dict(points=empty, colors=empty if colors is not None else None, normals=empty if normals is not None else None,
                    counts=np.zeros(0, np.int32), first_index=np.zeros(0, np.int32), row_of_point=row_of_point, origin=None, shift=None)
    index = np.nonzero(ok)[0]
    p = pts[index].astype(f64)
    v = np.floor((p - o) / float(h)).astype(np.int64)
    assert (v >= 0).all() and (v < 2 ** AXIS_BITS).all()
    key = (v[:, 2] << 42) | (v[:, 1] << 21) | v[:, 0]
    _, first, inverse = np.unique(key, return_index=True, return_inverse=True)       # first: positions in the finite subset, index ascends with them
    inverse = inverse.reshape(-1)
    rank = np.empty(len(first), np.int64)
    rank[np.argsort(first)] = np.arange(len(first))                                   # row of each unique key: the rank of its first appearance
    rows = rank[inverse]
    m = len(first)
    row_of_point[index] = rows
    counts = np.bincount(rows, minlength=m).astype(np.int64)
    first_index = np.empty(m, np.int32)
    first_index[rank] = index[first]
    single = counts == 1

    def sums(Q):
        S = np.zeros((m, 3), np.int64)
        np.add.at(S, rows, Q)
        return S

    c = counts.astype(f64)[:, None]
    Q = np.rint(np.ldexp(p - o, s)).astype(np.int64)
    assert (Q >= 0).all() and (Q <= 2 ** 32).all()
    out_p = (o + np.ldexp(sums(Q).astype(f64) / c, -s)).astype(f32)
    out_p[single] = pts[first_index[single]]
    out = dict(points=out_p, colors=None, normals=None, counts=counts.astype(np.int32), first_index=first_index, row_of_point=row_of_point,
               origin=o, shift=s)
    for name, a in attrs.items():
        Q = np.rint(np.ldexp(a[index].astype(f64), ATTR_SHIFT)).astype(np.int64)
        d = np.ldexp(sums(Q).astype(f64) / c, -ATTR_SHIFT)
        if name == "normals" and unit_normals:
            length = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
            with np.errstate(invalid="ignore", divide="ignore"):
                r = np.where(length[:, None] > 0.0, d / length[:, None], 0.0).astype(f32)
        else:
            r = d.astype(f32)
            r[single] = a[first_index[single]]
        out[name] = r
    return out


def mean_f64(points, row_of_point, m):
    """the float64 mean of the rounded points per row: what the error bound is against"""
    pts = np.asarray(points).astype(f32).astype(f64)
    ok = row_of_point >= 0
    S = np.zeros((m, 3))
    np.add.at(S, row_of_point[ok], pts[ok])
    return S / np.bincount(row_of_point[ok], minlength=m)[:, None]


def synthetic_colors(n):
    """float32 [n, 3] in [0, 1): a fixed pseudo-random colour per point"""
    return np.random.default_rng(29).random((n, 3)).astype(f32)
