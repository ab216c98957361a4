"""TSDF map of the SLAM loop: drop-in for BodySLAM_not_refactored/3DM/tsdf.py:5-52.

The reference's ``TSDF`` wraps Open3D's ``ScalableTSDFVolume(voxel_length=0.001, sdf_trunc=0.1, RGB8, volume_unit_resolution=32,
depth_sampling_stride=8)``: ``build_3D_map(rgbd, intrinsic, extrinsic)`` integrates a frame (3DM/slam.py:117,179 -- it passes the
accumulated pose as ``extrinsic``), ``extract_pcd`` / ``save_pcd`` read the surface points back (:126,191,195).  Same class, method
names and defaults here.  The voxels live in HBM (one contiguous block of res^3 x 5 fp32 per volume unit, allocated in slabs and
zero-filled once) and are integrated / extracted by the HIP kernels of csrc/tsdf.hip; which units exist is an open-addressing hash
table in HBM (Open3D: an unordered_map on the host), filled per frame from the strided depth sample exactly as Open3D does.  There is
one integration path: a pass over the map applies up to 64 frame records, ``build_3D_map`` is that pass on one record.  With the reference's parameters a
unit is 3.2 cm wide and a point opens the ~7^3 units within 0.1 m of it; a 640x480 frame of a surface at 12 cm touches ~1 600 units
= 1 GB of voxel state (tools/probes/tsdf_full_size.py; times in profiles/tsdf_one_path.txt),
metre-scale scenes proportionally more: the voxel store is sized for 288 GB of HBM.  Open3D is not vendored and not installable offline: parity against it is unpinned (oracle/tsdf_ref.py
restates the same algorithm in numpy; tests/ compare the two).  ``extract_pcd`` returns points, colours and normals, as Open3D's
``extract_point_cloud``; ``extract_mesh`` / ``save_mesh`` (tsdf.py:42-52, called on the last frame at 3DM/slam.py:189-193) run marching
cubes over every voxel cube on the device (bs_tsdf_mesh) with the case table of bodyslam_amd/marching_cubes.py and merge the
vertices of shared cube edges on the host.

``TSDF.raycast`` asks the map what a camera at a given pose sees (depth, colour, vertices, normals; bs_tsdf_raycast, one thread
per pixel through the unit table, every view of a call in one launch), and ``MAP`` is the drop-in for the reference's second class
(tsdf.py:56-107), which synthesises such a model frame after every integration and tracks the next frame against it
(``MAP.track_frame_to_model`` / ``track_and_integrate``: point-to-plane odometry on the ray-cast depth, rgbd_odometry.py).
"""
from __future__ import annotations

import copy
import ctypes as C
from dataclasses import dataclass
from typing import Optional, Sequence

import numpy as np
import torch

from . import _lib as L


@dataclass
class PinholeCameraIntrinsic:
    """o3d.camera.PinholeCameraIntrinsic(width, height, fx, fy, cx, cy)"""
    width: int
    height: int
    fx: float
    fy: float
    cx: float
    cy: float

    @property
    def intrinsic_matrix(self) -> np.ndarray:
        return np.array([[self.fx, 0.0, self.cx], [0.0, self.fy, self.cy], [0.0, 0.0, 1.0]])


@dataclass
class RGBDImage:
    """o3d.geometry.RGBDImage: colour u8 [H, W, 3] and depth fp32 [H, W] in metres (0 = no measurement)"""
    color: Optional[np.ndarray]
    depth: np.ndarray


def create_rgbd_from_color_and_depth(color_u8, depth_u16, depth_scale: float = 1000.0, depth_trunc: float = 3.0) -> RGBDImage:
    """o3d.geometry.RGBDImage.create_from_color_and_depth(..., convert_rgb_to_intensity=False) as the reference calls it
    (3DM/slam_utils.py:212-220): depth / depth_scale as fp32, values >= depth_trunc -> 0."""
    d = np.asarray(depth_u16).astype(np.float32) / np.float32(depth_scale)
    d[d >= np.float32(depth_trunc)] = 0.0
    return RGBDImage(None if color_u8 is None else np.ascontiguousarray(np.asarray(color_u8, dtype=np.uint8)), d)


@dataclass
class PointCloud:
    points: np.ndarray                      # [M, 3] float32
    colors: np.ndarray                      # [M, 3] float32 in [0, 1]
    normals: Optional[np.ndarray] = None    # [M, 3] float32, unit length (zero where the tsdf gradient vanishes)
    # (extract_pcd(host=False) fills the three fields with device tensors of the same shapes and rows)

    def compute_point_cloud_distance(self, target) -> np.ndarray:
        """o3d.geometry.PointCloud.compute_point_cloud_distance(target): for each point of this cloud the distance to the closest point
        of `target` (a PointCloud, or anything pointcloud.NearestNeighbours takes), float64 numpy [M].  Computed on the device in fp32
        (bodyslam_amd/pointcloud.py states the arithmetic); restated from Open3D's documented meaning, parity with Open3D unpinned."""
        from .pointcloud import point_cloud_distance
        return point_cloud_distance(self, target)[0].cpu().numpy().astype(np.float64)

    def estimate_normals(self, k: int = 30, radius: Optional[float] = None, direction=None, camera_location=None):
        """o3d.geometry.PointCloud.estimate_normals with a k-NN (or, with `radius`, hybrid) search: sets and returns ``self.normals`` --
        numpy float32 [M, 3] when `points` is numpy, a device tensor when extract_pcd(host=False) made the cloud.
        pointcloud.estimate_normals states the arithmetic and the sign rule; restated, parity with Open3D unpinned."""
        from .pointcloud import estimate_normals
        n = estimate_normals(self.points, k=k, radius=radius, direction=direction, camera_location=camera_location)
        self.normals = n.cpu().numpy() if isinstance(self.points, np.ndarray) else n
        return self.normals

    def orient_normals_consistent_tangent_plane(self, k: int):
        """o3d.geometry.PointCloud.orient_normals_consistent_tangent_plane(k): gives the cloud's normals (ValueError without them) one sign
        per surface by propagating it along the minimum spanning tree of the k-NN graph; sets and returns ``self.normals``, numpy for a
        numpy cloud, a device tensor otherwise.  pointcloud.orient_normals_consistent_tangent_plane states the rule and the departure
        from Open3D (no Delaunay edges: every component of the k-NN graph is oriented on its own); restated, parity with Open3D unpinned."""
        from .pointcloud import orient_normals_consistent_tangent_plane
        if self.normals is None:
            raise ValueError("orient_normals_consistent_tangent_plane needs the cloud's normals: estimate_normals first")
        n, _ = orient_normals_consistent_tangent_plane(self.points, self.normals, k)
        self.normals = n.cpu().numpy() if isinstance(self.points, np.ndarray) else n
        return self.normals

    def remove_statistical_outlier(self, nb_neighbors: int, std_ratio: float):
        """o3d.geometry.PointCloud.remove_statistical_outlier -> (the PointCloud of the kept rows -- points, colours and normals --, their
        indices int64 ascending: numpy for a numpy cloud, device tensors otherwise).  pointcloud.remove_statistical_outlier states the
        rule; restated, parity with Open3D unpinned."""
        from .pointcloud import remove_statistical_outlier
        ind, _ = remove_statistical_outlier(self.points, nb_neighbors=nb_neighbors, std_ratio=std_ratio)
        return self._kept(ind)

    def _kept(self, ind):
        """(the PointCloud of the rows `ind` (a device tensor), `ind`): numpy for a numpy cloud, device tensors otherwise"""
        def rows(a):
            if a is None:
                return None
            return a[ind.cpu().numpy()] if isinstance(a, np.ndarray) else a[ind.to(a.device)]
        ind_out = ind.cpu().numpy() if isinstance(self.points, np.ndarray) else ind
        return PointCloud(rows(self.points), rows(self.colors), rows(self.normals)), ind_out

    def remove_radius_outlier(self, nb_points: int, radius: float):
        """o3d.geometry.PointCloud.remove_radius_outlier -> (the PointCloud of the kept rows, their indices int64 ascending), as
        remove_statistical_outlier returns them: a point stays when more than nb_points points of the cloud, itself included, lie within
        `radius` of it.  pointcloud.remove_radius_outlier states the rule; restated, parity with Open3D unpinned."""
        from .pointcloud import remove_radius_outlier
        ind, _ = remove_radius_outlier(self.points, nb_points=nb_points, radius=radius)
        return self._kept(ind)

    def cluster_dbscan(self, eps: float, min_points: int):
        """o3d.geometry.PointCloud.cluster_dbscan -> labels int32 [M], -1 for noise: numpy for a numpy cloud, a device tensor otherwise.
        Deterministic: clusters are numbered by their smallest core point, a border point takes the smallest cluster number among its core
        neighbours.  pointcloud.cluster_dbscan states the rule; restated, parity with Open3D unpinned."""
        from .pointcloud import cluster_dbscan
        labels = cluster_dbscan(self.points, eps=eps, min_points=min_points)
        return labels.cpu().numpy() if isinstance(self.points, np.ndarray) else labels

    def compute_fpfh_feature(self, radius: float, max_nn: Optional[int] = 100):
        """o3d.pipelines.registration.compute_fpfh_feature(cloud, KDTreeSearchParamHybrid(radius, max_nn)) from the cloud's own normals
        (ValueError without them) -> fp32 [M, 33], one row per point: numpy for a numpy cloud, a device tensor otherwise.
        registration.compute_fpfh_feature states the arithmetic; restated, parity with Open3D unpinned."""
        from .registration import compute_fpfh_feature
        if self.normals is None:
            raise ValueError("compute_fpfh_feature needs the cloud's normals: estimate_normals first")
        f = compute_fpfh_feature(self.points, self.normals, radius, max_nn=max_nn)
        return f.cpu().numpy() if isinstance(self.points, np.ndarray) else f

    def voxel_down_sample(self, voxel_size: float) -> "PointCloud":
        """o3d.geometry.PointCloud.voxel_down_sample: one point per occupied cube of edge voxel_size, with the mean position, colour and
        normal of the cube's points (the plain mean: a normal is not re-normalised), rows in order of first appearance -- numpy for a
        numpy cloud, device tensors otherwise.  pointcloud.voxel_down_sample states the arithmetic; restated, parity with Open3D unpinned."""
        return self.voxel_down_sample_and_trace(voxel_size)[0]

    def voxel_down_sample_and_trace(self, voxel_size: float):
        """-> (the thinned PointCloud, row_of_point int32 [M] -- the output row of every input point, -1 for a non-finite one --, counts int32
        [m]): the role of o3d.geometry.PointCloud.voxel_down_sample_and_trace in tensor form.  Open3D's own trace (the cubic-id matrix and
        the index lists) is not built, and it takes no bounds: the grid is the one of pointcloud.voxel_down_sample."""
        from .pointcloud import voxel_down_sample
        r = voxel_down_sample(self.points, voxel_size, colors=self.colors, normals=self.normals)
        host = isinstance(self.points, np.ndarray)

        def out(a):
            return a.cpu().numpy() if host and a is not None else a
        return PointCloud(out(r.points), out(r.colors), out(r.normals)), out(r.row_of_point), out(r.counts)


@dataclass(init=False)
class TriangleMesh:
    vertices: np.ndarray                    # [V, 3] float32
    vertex_colors: np.ndarray               # [V, 3] float32 in [0, 1]
    triangles: np.ndarray                   # [T, 3] int32, wound so that the normal points from tsdf < 0 to tsdf > 0
    # (extract_mesh(host=False) fills the fields with device tensors of the same shapes and rows)
    # The normals are two trailing optional arguments of the constructor and plain attributes, not dataclass fields: the field list is the
    # mesh's identity (tests/test_mesh_scene_cpu.py pins it), the normals are derived from it and go stale when it changes.
    triangle_normals = None                 # [T, 3] float32, set by compute_triangle_normals
    vertex_normals = None                   # [V, 3] float32, set by compute_vertex_normals

    def __init__(self, vertices, vertex_colors, triangles, triangle_normals=None, vertex_normals=None):
        self.vertices, self.vertex_colors, self.triangles = vertices, vertex_colors, triangles
        self.triangle_normals, self.vertex_normals = triangle_normals, vertex_normals

    # ---- topology and clean-up: thin wrappers of bodyslam_amd/mesh.py, which states the rules; restated from Open3D's documentation, parity with
    # Open3D unpinned.  Results are numpy for a mesh of numpy arrays and device tensors for a mesh of device tensors.
    def _host(self) -> bool:
        return isinstance(self.vertices, np.ndarray)

    def _out(self, x):
        return x.cpu().numpy() if self._host() and isinstance(x, torch.Tensor) else x

    def edge_topology(self):
        """-> mesh.MeshEdges: the unique edges in the order of their first half-edge, the triangles on each, how many run it forward"""
        from .mesh import MeshEdges, edge_topology
        e = edge_topology(self.vertices, self.triangles)
        return MeshEdges(*(self._out(x) for x in (e.edges, e.edge_count, e.edge_forward, e.edge_first_triangle, e.edge_of_half)),
                         e.n_invalid_triangles, e.n_vertices)

    def get_non_manifold_edges(self, allow_boundary_edges: bool = True):
        """o3d get_non_manifold_edges: int32 [n, 2], the edges with more than two triangles (allow_boundary_edges=False: without exactly two)"""
        from .mesh import edge_topology
        return self._out(edge_topology(self.vertices, self.triangles).get_non_manifold_edges(allow_boundary_edges))

    def get_boundary_edges(self):
        """int32 [n, 2]: the edges with exactly one triangle -- the rims of the holes"""
        from .mesh import edge_topology
        return self._out(edge_topology(self.vertices, self.triangles).get_boundary_edges())

    def is_edge_manifold(self, allow_boundary_edges: bool = True) -> bool:
        from .mesh import edge_topology
        return edge_topology(self.vertices, self.triangles).is_edge_manifold(allow_boundary_edges)

    def is_consistently_oriented(self) -> bool:
        """every edge of two triangles is run once in each direction (the test of the winding as it stands; is_orientable asks whether it
        can be made so, orient_triangles makes it so)"""
        from .mesh import edge_topology
        return edge_topology(self.vertices, self.triangles).is_consistently_oriented()

    def is_orientable(self) -> bool:
        """o3d is_orientable: every component of triangles joined through two-triangle edges can be wound consistently"""
        from .mesh import is_orientable
        return is_orientable(self.vertices, self.triangles)

    def orient_triangles(self):
        """o3d orient_triangles, returning a new mesh -> (TriangleMesh with every orientable component wound like its first triangle -- the
        normals are not carried: they would be stale --, flipped bool [T], orientable bool).  A component that cannot be wound
        consistently is left as it is and makes orientable False.  mesh.orient_triangles states the rule."""
        from .mesh import orient_triangles
        t, flipped, ok = orient_triangles(self.vertices, self.triangles)
        return TriangleMesh(self.vertices, self.vertex_colors, self._out(t)), self._out(flipped), ok

    def is_closed(self) -> bool:
        """every edge has exactly two triangles; is_watertight() also wants vertex-manifoldness and no self-intersection, and with
        is_consistently_oriented() it is the precondition of a signed distance and of get_volume()"""
        from .mesh import edge_topology
        return edge_topology(self.vertices, self.triangles).is_closed()

    # ---- is the mesh a solid (mesh.py states the rules; csrc/mesh_solid.hip) ----------------------------------------------------------------
    def get_non_manifold_vertices(self):
        """o3d get_non_manifold_vertices: int32 [n], the vertices whose triangles form more than one fan (a bow-tie), ascending; the end
        points of an edge with three or more triangles are not reported for that reason alone"""
        from .mesh import get_non_manifold_vertices
        return self._out(get_non_manifold_vertices(self.vertices, self.triangles))

    def is_vertex_manifold(self) -> bool:
        from .mesh import is_vertex_manifold
        return is_vertex_manifold(self.vertices, self.triangles)

    def get_self_intersecting_triangles(self, method: str = "auto", cells: Optional[int] = None):
        """o3d get_self_intersecting_triangles: int32 [n, 2], the pairs i < j of triangles without a common vertex index that have a point
        in common (touching counts), ascending"""
        from .mesh import get_self_intersecting_triangles
        return self._out(get_self_intersecting_triangles(self.vertices, self.triangles, method=method, cells=cells))

    def is_self_intersecting(self, method: str = "auto", cells: Optional[int] = None) -> bool:
        from .mesh import is_self_intersecting
        return is_self_intersecting(self.vertices, self.triangles, method=method, cells=cells)

    def get_intersecting_triangles(self, other: "TriangleMesh", method: str = "auto", cells: Optional[int] = None):
        """int32 [n, 2]: the pairs (triangle of this mesh, triangle of `other`) that have a point in common, ascending"""
        from .mesh import get_intersecting_triangles
        return self._out(get_intersecting_triangles(self, other, method=method, cells=cells))

    def is_intersecting(self, other: "TriangleMesh", method: str = "auto", cells: Optional[int] = None) -> bool:
        """o3d is_intersecting(other)"""
        from .mesh import is_intersecting
        return is_intersecting(self, other, method=method, cells=cells)

    def is_watertight(self) -> bool:
        """o3d is_watertight: every edge has exactly two triangles, every vertex one fan, and no two triangles intersect -- what
        compute_signed_distance, compute_occupancy and evaluate_reconstruction_signed assume of the mesh"""
        from .mesh import is_watertight
        return is_watertight(self.vertices, self.triangles)

    def component_volumes(self):
        """-> (triangle_clusters int32 [T], signed volume float64 [C] of every cluster, positive when wound outwards, NaN when the cluster
        is open or not consistently oriented)"""
        from .mesh import component_volumes
        return tuple(self._out(x) for x in component_volumes(self.vertices, self.triangles))

    def get_volume(self) -> float:
        """o3d get_volume: ValueError unless the mesh is watertight and consistently oriented"""
        from .mesh import get_volume
        return get_volume(self.vertices, self.triangles)

    def orient_outward(self):
        """orient_triangles(), then every closed cluster with a negative signed volume turned inside out -> (a new TriangleMesh -- the
        normals are not carried: they would be stale --, flipped bool [T], solid bool [C]: the clusters that have a volume)"""
        from .mesh import orient_outward
        t, flipped, solid = orient_outward(self.vertices, self.triangles)
        return TriangleMesh(self.vertices, self.vertex_colors, self._out(t)), self._out(flipped), self._out(solid)

    def check_solid(self):
        """-> mesh.SolidReport: the verdicts, the counts behind them and the volume when the mesh has one"""
        from .mesh import check_solid
        return check_solid(self.vertices, self.triangles)

    def cluster_connected_triangles(self):
        """o3d cluster_connected_triangles -> (triangle_clusters int32 [T], cluster_n_triangles int32 [C], cluster_area float64 [C]); triangles
        that share an edge are connected, clusters are numbered by their first triangle"""
        from .mesh import cluster_connected_triangles
        return tuple(self._out(x) for x in cluster_connected_triangles(self.vertices, self.triangles))

    def get_surface_area(self) -> float:
        from .mesh import get_surface_area
        return get_surface_area(self.vertices, self.triangles)

    def remove_triangles_by_mask(self, mask) -> "TriangleMesh":
        """o3d remove_triangles_by_mask, returning a new mesh: the triangles whose mask is True leave, the vertices stay"""
        from .mesh import remove_triangles_by_mask
        return remove_triangles_by_mask(self, mask)[0]

    def remove_unreferenced_vertices(self) -> "TriangleMesh":
        """o3d remove_unreferenced_vertices, returning a new mesh"""
        from .mesh import remove_unreferenced_vertices
        return remove_unreferenced_vertices(self)[0]

    def remove_small_components(self, min_triangles: Optional[int] = None, min_area: Optional[float] = None, keep_largest: bool = False):
        """-> (TriangleMesh without the clusters of fewer than min_triangles triangles or less than min_area area -- keep_largest: without all
        but the largest --, vertex_map int32 [V], triangle_map int32 [T]: the new row of every old row or -1).  Order-preserving."""
        from .mesh import remove_small_components
        return remove_small_components(self, min_triangles=min_triangles, min_area=min_area, keep_largest=keep_largest)

    def compute_triangle_normals(self):
        """o3d compute_triangle_normals: sets and returns ``triangle_normals``, the unit face normals (zero for a degenerate triangle)"""
        from .mesh import compute_triangle_normals
        self.triangle_normals = self._out(compute_triangle_normals(self.vertices, self.triangles))
        return self.triangle_normals

    def compute_vertex_normals(self):
        """o3d compute_vertex_normals: sets and returns ``vertex_normals``, area-weighted"""
        from .mesh import compute_vertex_normals
        self.vertex_normals = self._out(compute_vertex_normals(self.vertices, self.triangles))
        return self.vertex_normals

    def _smoothed(self, v, c) -> "TriangleMesh":
        return TriangleMesh(self._out(v), self.vertex_colors if c is None else self._out(c), self.triangles)

    def filter_smooth_laplacian(self, number_of_iterations: int = 1, lambda_filter: float = 0.5, colors: bool = False) -> "TriangleMesh":
        """o3d filter_smooth_laplacian -> a new mesh (normals are not carried: they would be stale); colors: smooth the vertex colours too"""
        from .mesh import filter_smooth_laplacian
        if not isinstance(colors, bool):
            raise ValueError(f"colors {colors!r}: expected a bool")
        return self._smoothed(*filter_smooth_laplacian(self.vertices, self.triangles, number_of_iterations, lambda_filter,
                                                       vertex_colors=self.vertex_colors if colors else None))

    def filter_smooth_taubin(self, number_of_iterations: int = 1, lambda_filter: float = 0.5, mu: float = -0.53, colors: bool = False) -> "TriangleMesh":
        """o3d filter_smooth_taubin -> a new mesh: per iteration the lambda step, then the mu step"""
        from .mesh import filter_smooth_taubin
        if not isinstance(colors, bool):
            raise ValueError(f"colors {colors!r}: expected a bool")
        return self._smoothed(*filter_smooth_taubin(self.vertices, self.triangles, number_of_iterations, lambda_filter, mu,
                                                    vertex_colors=self.vertex_colors if colors else None))

    def sample_points_uniformly(self, number_of_points: int, seed: int = 0, host: Optional[bool] = None):
        """o3d.geometry.TriangleMesh.sample_points_uniformly -> (the PointCloud of number_of_points samples drawn uniformly by area -- points,
        colours interpolated from vertex_colors with the sample's barycentric weights, normals = the unit face normal --, the int32 triangle
        index of every sample).  host: numpy arrays (True) or device tensors (False); None: numpy for a mesh of numpy arrays.  A mesh
        without a triangle of positive area returns an empty cloud.  pointcloud.sample_mesh states the arithmetic: a sample depends on
        (seed, its number) alone, the same bits in every run; restated, parity with Open3D unpinned."""
        from .pointcloud import sample_mesh
        if host is None:
            host = isinstance(self.vertices, np.ndarray)
        pts, col, nrm, idx = sample_mesh(self.vertices, self.triangles, number_of_points, vertex_colors=self.vertex_colors, seed=seed)

        def out(a):
            return a.cpu().numpy() if host and a is not None else a
        return PointCloud(out(pts), out(col), out(nrm)), out(idx)


@dataclass
class RaycastFrame:
    """What ``TSDF.raycast`` returns: device tensors, [n, H, W, ...] for a sequence of views, [H, W, ...] for a single 4x4."""
    depth: torch.Tensor                         # fp32 metres (camera-frame z of the surface point), 0 = no surface
    color: Optional[torch.Tensor] = None        # u8 x 3
    vertex: Optional[torch.Tensor] = None       # fp32 x 3, world coordinates, 0 where there is no surface
    normal: Optional[torch.Tensor] = None       # fp32 x 3, unit length, 0 where there is no surface (or the tsdf gradient vanishes)

    def _view(self, t: torch.Tensor, i: int) -> torch.Tensor:
        if self.depth.dim() == 2:
            if i != 0:
                raise IndexError(f"view {i} of a single-view RaycastFrame")
            return t
        return t[i]

    def to_rgbd(self, i: int = 0) -> RGBDImage:
        """view i as an RGBDImage of device tensors: straight into build_3D_map, rgbd_odometry or a comparison"""
        return RGBDImage(None if self.color is None else self._view(self.color, i), self._view(self.depth, i))

    def depth_u16(self, depth_scale: float = 1000.0) -> torch.Tensor:
        """depth * depth_scale rounded to nearest as uint16 values in int16 storage (values above 65 535 saturate): the layout
        evaluation.evaluate_depth reads, 0 = no surface"""
        v = torch.clamp(torch.round(self.depth.to(torch.float64) * float(depth_scale)), 0.0, 65535.0).to(torch.int32)
        return torch.where(v >= 32768, v - 65536, v).to(torch.int16)


@dataclass
class TrackingResult:
    """What ``MAP.track_frame_to_model`` returns (Open3D: OdometryResult)"""
    transformation: np.ndarray                  # 4x4 float64: the input frame -> the camera raycast_frame was cast from
    pose: np.ndarray                            # 4x4 float64: that camera's pose composed with it = the frame's camera -> world
    inliers: int                                # of the last step (the finest level)
    cost: float                                 # sum of huber(r) over them
    fitness: float                              # inliers / (H * W)


BATCH_MAX = 64              # frames per pass of build_3D_map_batch (BS_TSDF_BATCH_MAX: one bit per frame in a unit's mask)
_OFF = 1 << 20              # unit indices are packed as three 21-bit fields (csrc/tsdf.hip ts_pack)


class TSDF:
    def __init__(self, voxel_length: float = 0.001, sdf_trunc: float = 0.1, volume_unit_resolution: int = 32,
                 depth_sampling_stride: int = 8, device: int = 0, slab_bytes: int = 1 << 30, max_units: Optional[int] = None):
        """max_units bounds the map (default: as many 32^3-voxel-sized blocks as fit 64 GB); the unit table is 4x that, a power of two."""
        self.voxel_length, self.sdf_trunc = float(voxel_length), float(sdf_trunc)
        self.res, self.stride = int(volume_unit_resolution), int(depth_sampling_stride)
        self.unit_length = self.voxel_length * self.res
        self.dev = torch.device("cuda", device)
        L.init(device)
        self.unit_floats = self.res ** 3 * 5
        self.slab_units = max(1, slab_bytes // (self.unit_floats * 4))
        self.max_units = int(max_units) if max_units else max(1024, min(1 << 20, (64 << 30) // (self.unit_floats * 4)))
        self.table_cap = 256
        while self.table_cap < 4 * self.max_units:
            self.table_cap *= 2
        self.max_slabs = -(-self.max_units // self.slab_units)
        self._alloc_state()

    def _alloc_state(self):
        d = self.dev
        self.slabs = []                                                   # fp32 [slab_units, unit_floats] tensors, zero-filled
        self.slab_base = torch.zeros(self.max_slabs, dtype=torch.int64, device=d)
        self.table_keys = torch.full((self.table_cap,), -1, dtype=torch.int64, device=d)
        self.table_slots = torch.full((self.table_cap,), -1, dtype=torch.int32, device=d)
        self.unit_index = torch.zeros(self.max_units, 3, dtype=torch.int32, device=d)
        self.counters = torch.zeros(3, dtype=torch.int32, device=d)
        self.touched = torch.zeros(self.max_units, dtype=torch.int32, device=d)
        self._alloc_pass_scratch()
        self.n_units, self.frames_integrated = 0, 0
        self._max_new_per_frame, self._frames_since_sync = 0, 0

    def _alloc_pass_scratch(self):
        """what a pass over the map works in and leaves behind clean: the table's record masks (zero between passes), the masks per
        block and the frame records"""
        self.table_fmask = torch.zeros(self.table_cap, dtype=torch.int64, device=self.dev)
        self.unit_mask = torch.zeros(self.max_units, dtype=torch.int64, device=self.dev)
        self.frames_dev = torch.zeros(BATCH_MAX * 256, dtype=torch.uint8, device=self.dev)          # BS_TSDF_FRAME_BYTES per frame

    # ---- block capacity ------------------------------------------------------------------------------
    @property
    def alloc_units(self) -> int:
        """blocks that exist (zero-filled slabs): the unit table never hands out more"""
        return min(len(self.slabs) * self.slab_units, self.max_units)

    def reserve(self, units: int) -> None:
        """make sure at least `units` blocks exist (new slabs are allocated and zero-filled here, not inside a frame)"""
        units = min(int(units), self.max_units)
        while len(self.slabs) * self.slab_units < units:
            self.slabs.append(torch.zeros(self.slab_units, self.unit_floats, device=self.dev))
            self.slab_base[len(self.slabs) - 1] = self.slabs[-1].data_ptr()

    def reserve_ahead(self, n_frames: int) -> None:
        """capacity for `n_frames` un-synchronised frames: the known unit count + 2 048 (a first view of a scene opens ~1 500 units at
        endoscopic range) + per frame four times what the frames of the last stream opened on average, at least 128 (measured on the
        bench's synthetic sequence: ~65).  A stream that still runs out is reported by sync() -- 288 GB of HBM is what makes the
        generous bound affordable (a block is 655 KB)."""
        self.reserve(self.n_units + 2048 + n_frames * max(128, 4 * self._max_new_per_frame))

    def n_units_known(self) -> int:
        return self.n_units

    def discover(self, rgbd: "RGBDImage", intrinsic: "PinholeCameraIntrinsic", extrinsic) -> None:
        """unit discovery of a frame WITHOUT integrating it (no round trip): the units it needs enter the table, without blocks.
        ``reserve_discovered()`` then makes the missing blocks -- two cheap passes over a batch of frames replace a guess at how
        many units a stream will open."""
        self._discover([rgbd], intrinsic, [extrinsic])
        self.table_fmask.zero_()              # no pass follows that would clear it: a stale bit would name a frame of the next pass
        self._frames_since_sync += 1

    def reserve_discovered(self, margin: int = 256) -> int:
        """after a run of discover() calls: one round trip for the unit count and the number of table entries still without a block;
        allocates what is missing (+ margin), so that the frames can be streamed (each takes its blocks as it is integrated), and
        clears the overflow flag.  Returns the blocks added."""
        n_units = int(self.counters[0])
        missing = int(((self.table_keys != -1) & (self.table_slots < 0)).sum())
        before = self.alloc_units
        self.reserve(n_units + missing + margin)
        self.counters[2] = 0
        self.n_units = n_units
        self._frames_since_sync = 0
        return self.alloc_units - before

    def sync(self):
        """the round trip a stream of build_3D_map(sync=False) calls owes: unit counts, and the overflow check"""
        n_units, n_touched, overflow = (int(v) for v in self.counters.cpu())
        if overflow:
            self.counters[2] = 0
            if overflow == 3:          # tsdf_apply_batch_kernel<true>: the removal was skipped there, no weight went below 0
                raise L.BodySlamHipError("TSDF: a frame was removed that the voxel never held (deintegrate / apply_batch need the images and the "
                                         "extrinsic the frame was integrated with)")
            raise L.BodySlamHipError("TSDF: " + ("unit table full" if overflow == 1 else
                                                 f"a frame needed more than the {self.alloc_units} blocks that existed (reserve() more ahead of a "
                                                 f"stream, or raise max_units={self.max_units})"))
        self._max_new_per_frame = max(self._max_new_per_frame, (n_units - self.n_units) // max(self._frames_since_sync, 1) + 1)
        self._frames_since_sync = 0
        self.n_units, self.last_units = n_units, n_touched
        return n_units, n_touched

    # ---- the reference's surface -----------------------------------------------------------------
    def build_3D_map(self, rgbd: RGBDImage, intrinsic: PinholeCameraIntrinsic, extrinsic, sync: bool = True) -> None:
        """ScalableTSDFVolume.integrate(rgbd, intrinsic, extrinsic): a pass of one record.  sync=True (one frame at a time, as the
        reference calls it): the blocks the frame needs are counted (one round trip) and made first.  sync=False: nothing is read
        back -- the frame is enqueued against the blocks that exist (reserve / reserve_ahead) and ``sync()`` later collects the counts
        and the overflow flag."""
        self._batch_pass([rgbd], intrinsic, [extrinsic], None, sync=sync)

    def build_3D_map_batch(self, rgbds: Sequence["RGBDImage"], intrinsic: "PinholeCameraIntrinsic", extrinsics) -> None:
        """``build_3D_map`` for a run of frames, in order, as ONE pass over the map (csrc/tsdf.hip, "Integrate for a batch of records"):
        every voxel the run touches is loaded once, takes its frames in ascending order in registers and is stored once.  The blocks
        end up bit for bit as the frame-by-frame calls leave them; the cost is three launches and one round trip (the block
        reservation) per 64 frames instead of per frame.  Device images (torch tensors) are used in place."""
        n = len(rgbds)
        assert len(extrinsics) == n
        for a in range(0, n, BATCH_MAX):
            self._batch_pass(rgbds[a:a + BATCH_MAX], intrinsic, extrinsics[a:a + BATCH_MAX], None)

    def _discover(self, chunk, intrinsic: "PinholeCameraIntrinsic", extrinsics):
        """the records of at most BATCH_MAX frames go to the device and their units into the table: afterwards bit f of table_fmask
        marks the units record f touches.  Returns (records, H, W, the device images): the records point at the images, so the
        caller holds on to them until everything that reads the records is enqueued."""
        lib, st = L.load_library(), L.stream_ptr()
        if not self.slabs:
            self.reserve(1)
        K = np.array([intrinsic.fx, intrinsic.fy, intrinsic.cx, intrinsic.cy], dtype=np.float64)
        m = len(chunk)
        depth = [self._image(r.depth, torch.float32) for r in chunk]
        has_color = chunk[0].color is not None
        assert all((r.color is not None) == has_color for r in chunk), "either every frame of a batch has a colour image or none"
        color = [self._image(r.color, torch.uint8) for r in chunk] if has_color else None
        H, W = depth[0].shape
        assert all(d.shape == (H, W) for d in depth)
        E = np.ascontiguousarray(np.stack([np.asarray(self._np(e), dtype=np.float64) for e in extrinsics]).reshape(m, 16))
        P = np.ascontiguousarray(np.linalg.inv(E.reshape(m, 4, 4)).reshape(m, 16))
        dptr = np.array([d.data_ptr() for d in depth], dtype=np.uint64)
        cptr = np.array([c.data_ptr() for c in color], dtype=np.uint64) if has_color else None
        L.check(lib.bs_tsdf_frames_upload(dptr.ctypes.data_as(C.c_void_p), cptr.ctypes.data_as(C.c_void_p) if has_color else None,
                                          K.ctypes.data_as(C.c_void_p), E.ctypes.data_as(C.c_void_p), P.ctypes.data_as(C.c_void_p), m,
                                          L.p(self.frames_dev), st), "bs_tsdf_frames_upload")
        L.check(lib.bs_tsdf_touch_batch(L.p(self.frames_dev), m, H, W, self.stride, self.unit_length, self.sdf_trunc, L.p(self.table_keys),
                                        L.p(self.table_fmask), self.table_cap, L.p(self.counters), st), "bs_tsdf_touch_batch")
        return m, H, W, (depth, color)

    def _batch_pass(self, chunk, intrinsic: "PinholeCameraIntrinsic", extrinsics, remove, sync: bool = True) -> None:
        """one pass over the map for at most BATCH_MAX records: discovery, the round trip that makes the blocks (sync=False: none, the
        blocks that exist have to do and ``sync()`` tells whether they did), the update.
        remove = None: every record is added (bs_tsdf_integrate_batch); else a bool per record, True = taken out (bs_tsdf_update_batch)"""
        lib, st = L.load_library(), L.stream_ptr()
        m, H, W, images = self._discover(chunk, intrinsic, extrinsics)
        if sync:
            # the one round trip of the pass: the units that have blocks, the units of this pass that need one
            # (+ the overflow flag the discovery may have raised: 1 = unit table full)
            need = torch.stack([self.counters[0].to(torch.int64), ((self.table_fmask != 0) & (self.table_slots < 0)).sum(),
                                self.counters[2].to(torch.int64)]).cpu()
            n_units = int(need[0]) + int(need[1])
            if int(need[2]) == 1 or n_units > self.max_units:
                # nothing of this pass has been integrated yet: clear the flag and the pass's record bits, then refuse
                self.counters[2] = 0
                self.table_fmask.zero_()
                raise L.BodySlamHipError("TSDF: " + ("unit table full" if int(need[2]) == 1 else
                                                     f"the batch needs {n_units} volume units, more than max_units={self.max_units}")
                                         + "; construct TSDF with a larger max_units")
            self.reserve(n_units)
            # every unit of the pass has a block once it has run, so the count is known without another round trip -- extract_pcd /
            # extract_mesh right after it see the whole map
            self._max_new_per_frame = max(self._max_new_per_frame, -(-(n_units - self.n_units) // m))
            self.n_units, self._frames_since_sync = n_units, 0
        else:
            self._frames_since_sync += m
        args = (L.p(self.frames_dev), m, H, W, L.p(self.table_keys), L.p(self.table_slots), L.p(self.table_fmask), self.table_cap, L.p(self.unit_index),
                self.alloc_units, L.p(self.counters), L.p(self.touched), L.p(self.unit_mask), L.p(self.slab_base), self.slab_units, self.res,
                self.voxel_length, self.sdf_trunc)
        if remove is None:
            L.check(lib.bs_tsdf_integrate_batch(*args, st), "bs_tsdf_integrate_batch")
            removed = 0
        else:
            mask = sum(1 << f for f in range(m) if remove[f])
            L.check(lib.bs_tsdf_update_batch(*args, mask, st), "bs_tsdf_update_batch")
            removed = sum(1 for f in range(m) if remove[f])
        self.frames_integrated += m - 2 * removed
        del images                            # (enqueued: the allocator frees in stream order)

    def apply_batch(self, rgbds: Sequence["RGBDImage"], intrinsic: "PinholeCameraIntrinsic", extrinsics, remove: Sequence[bool]) -> None:
        """Records with a sign: ``remove[k]`` False integrates record k as ``build_3D_map_batch`` does, True takes it out of the map
        again -- it must carry the images and the extrinsic it was integrated with.  Records are applied in the given order, in chunks
        of at most BS_TSDF_BATCH_MAX consecutive records; each chunk is one discovery, one round trip and one pass that loads
        every touched voxel once (csrc/tsdf.hip, "frames taken out again"), with ``build_3D_map_batch``'s capacity checks before
        anything of the chunk is applied.  Units are never freed: a unit whose voxels all returned to weight 0 keeps its (all-zero)
        block, which extract_pcd / extract_mesh / raycast ignore.  Removing a frame the map never held is reported by ``sync()``."""
        n = len(rgbds)
        assert len(extrinsics) == n and len(remove) == n
        remove = [bool(r) for r in remove]
        for a in range(0, n, BATCH_MAX):
            self._batch_pass(rgbds[a:a + BATCH_MAX], intrinsic, extrinsics[a:a + BATCH_MAX], remove[a:a + BATCH_MAX])

    def deintegrate(self, rgbd: "RGBDImage", intrinsic: "PinholeCameraIntrinsic", extrinsic, sync: bool = True) -> None:
        """take one frame out of the map: the inverse of ``build_3D_map(rgbd, intrinsic, extrinsic)`` with the same arguments"""
        self.apply_batch([rgbd], intrinsic, [extrinsic], [True])
        if sync:
            self.sync()

    def _image(self, x, dtype) -> torch.Tensor:
        t = x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(x)))
        return t.to(device=self.dev, dtype=dtype).contiguous()

    def build_copy_3D_map(self, rgbd, intrinsic, extrinsic) -> "TSDF":
        other = copy.copy(self)
        for name in ("table_keys", "table_slots", "unit_index", "counters", "touched"):
            setattr(other, name, getattr(self, name).clone())
        other._alloc_pass_scratch()
        other.slabs = [s.clone() for s in self.slabs]
        other.slab_base = torch.zeros_like(self.slab_base)
        for n, sl in enumerate(other.slabs):
            other.slab_base[n] = sl.data_ptr()
        other.build_3D_map(rgbd, intrinsic, extrinsic)
        return other

    def extract_pcd(self, host: bool = True) -> PointCloud:
        """host=False: the PointCloud's fields are device tensors holding the same rows, so a map of millions of points is evaluated where
        it lies (evaluation.evaluate_reconstruction).  In either form the rows of one volume unit come out in the order the extraction's
        atomics gave, which differs from call to call."""
        U = self.n_units
        if U == 0:
            if not host:
                return PointCloud(*(torch.zeros(0, 3, device=self.dev) for _ in range(3)))
            return PointCloud(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.float32), np.zeros((0, 3), np.float32))
        count = torch.zeros(U, dtype=torch.int32, device=self.dev)
        lib = L.load_library()
        args = (L.p(self.unit_index), U, L.p(self.table_keys), L.p(self.table_slots), self.table_cap, L.p(self.slab_base), self.slab_units, self.res,
                self.voxel_length, L.p(count))
        L.check(lib.bs_tsdf_extract(*args, None, None, None, None, L.stream_ptr()), "bs_tsdf_extract")
        counts = count.cpu().numpy().astype(np.int64)
        total = int(counts.sum())
        pts = torch.empty(max(total, 1), 3, device=self.dev)
        cols = torch.empty(max(total, 1), 3, device=self.dev)
        nrm = torch.empty(max(total, 1), 3, device=self.dev)
        off = torch.from_numpy(np.concatenate([[0], np.cumsum(counts)[:-1]]).astype(np.int64)).to(self.dev)
        L.check(lib.bs_tsdf_extract(*args, L.p(off), L.p(pts), L.p(cols), L.p(nrm), L.stream_ptr()), "bs_tsdf_extract")
        if not host:
            return PointCloud(pts[:total], cols[:total], nrm[:total])
        return PointCloud(pts[:total].cpu().numpy(), cols[:total].cpu().numpy(), nrm[:total].cpu().numpy())

    def save_pcd(self, saving_path: str) -> None:
        write_ply(saving_path, self.extract_pcd())

    def _empty_mesh(self, host: bool) -> TriangleMesh:
        if not host:
            return TriangleMesh(torch.zeros(0, 3, device=self.dev), torch.zeros(0, 3, device=self.dev),
                                torch.zeros(0, 3, dtype=torch.int32, device=self.dev))
        return TriangleMesh(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32))

    def extract_mesh(self, host: bool = True) -> TriangleMesh:
        """ScalableTSDFVolume.extract_triangle_mesh(): marching cubes over every voxel cube whose eight corners carry weight.  host=False:
        the TriangleMesh's fields are device tensors holding the same rows, so the mesh is cleaned where it lies (bodyslam_amd/mesh.py)."""
        from . import marching_cubes as MC
        U = self.n_units
        if U == 0:
            return self._empty_mesh(host)
        if getattr(self, "_mc_tab", None) is None:
            tab = np.concatenate([MC.TRI_TABLE.reshape(-1), np.array(MC.EDGES, dtype=np.int32).reshape(-1)]).astype(np.int32)
            self._mc_tab = torch.from_numpy(tab).to(self.dev)
        lib = L.load_library()
        count = torch.zeros(U, dtype=torch.int32, device=self.dev)
        err = torch.zeros(1, dtype=torch.int32, device=self.dev)
        args = (L.p(self.unit_index), U, L.p(self.table_keys), L.p(self.table_slots), self.table_cap, L.p(self.slab_base), self.slab_units, self.res,
                self.voxel_length, L.p(self._mc_tab), int(MC.TRI_TABLE.shape[1]), L.p(count))
        L.check(lib.bs_tsdf_mesh(*args, None, None, None, None, L.p(err), L.stream_ptr()), "bs_tsdf_mesh")
        counts = count.cpu().numpy().astype(np.int64)
        total = int(counts.sum())
        if total == 0:
            return self._empty_mesh(host)
        off = torch.from_numpy(np.concatenate([[0], np.cumsum(counts)[:-1]]).astype(np.int64)).to(self.dev)
        verts = torch.empty(3 * total, 3, device=self.dev)
        cols = torch.empty(3 * total, 3, device=self.dev)
        keys = torch.empty(3 * total, dtype=torch.int64, device=self.dev)
        L.check(lib.bs_tsdf_mesh(*args, L.p(off), L.p(verts), L.p(cols), L.p(keys), L.p(err), L.stream_ptr()), "bs_tsdf_mesh")
        if int(err.cpu()):
            raise L.BodySlamHipError("TSDF.extract_mesh: the map spans more than 2^20 voxels along an axis (vertex identity overflow)")
        # equal edge identities are one vertex (every cube that shares the edge computed the same position)
        # (merged on the device: a radix sort of the keys; on the host np.unique took 1 s for 17 M corners -- longer than a 256-frame loop)
        uniq, inverse = torch.unique(keys, sorted=True, return_inverse=True)
        first = torch.full((uniq.shape[0],), keys.shape[0], dtype=torch.int64, device=self.dev)
        first.scatter_reduce_(0, inverse, torch.arange(keys.shape[0], device=self.dev), reduce="amin")      # the first corner of every vertex
        if not host:
            return TriangleMesh(verts[first], cols[first], inverse.view(-1, 3).to(torch.int32).contiguous())
        return TriangleMesh(verts[first].cpu().numpy(), cols[first].cpu().numpy(), inverse.view(-1, 3).to(torch.int32).cpu().numpy())

    def save_mesh(self, saving_path: str) -> None:
        write_ply_mesh(saving_path, self.extract_mesh())

    def raycast(self, intrinsic: PinholeCameraIntrinsic, extrinsic, depth_min: float = 0.0, depth_max: float = 3.0, vertex: bool = False,
                normal: bool = False, color: bool = True) -> RaycastFrame:
        """The map as a camera sees it: ``extrinsic`` (world -> camera, the convention of build_3D_map -- raycast(extrinsic=E)
        re-renders what build_3D_map(..., E) integrated) is one 4x4, or a sequence / [n, 4, 4] array or tensor of them; all views go
        down in one call.  Rays run from depth_min to depth_max metres.  Nothing is read back and nothing waits: the call may follow
        build_3D_map(sync=False) frames directly, and the frame's tensors are valid in stream order."""
        if isinstance(extrinsic, (list, tuple)):
            E = np.stack([self._np(e) for e in extrinsic]) if len(extrinsic) else np.zeros((0, 4, 4))
        else:
            E = self._np(extrinsic)
        E = np.asarray(E, dtype=np.float64)
        single = E.ndim == 2
        E = np.ascontiguousarray(E.reshape(-1, 4, 4))
        n, H, W = E.shape[0], int(intrinsic.height), int(intrinsic.width)
        K = np.array([intrinsic.fx, intrinsic.fy, intrinsic.cx, intrinsic.cy], dtype=np.float64)
        d = self.dev
        out_d = torch.empty(n, H, W, dtype=torch.float32, device=d)
        out_v = torch.empty(n, H, W, 3, dtype=torch.float32, device=d) if vertex else None
        out_n = torch.empty(n, H, W, 3, dtype=torch.float32, device=d) if normal else None
        out_c = torch.empty(n, H, W, 3, dtype=torch.uint8, device=d) if color else None
        L.check(L.load_library().bs_tsdf_raycast(K.ctypes.data_as(C.c_void_p), E.ctypes.data_as(C.c_void_p), n, H, W, float(depth_min), float(depth_max),
                                                 L.p(self.table_keys), L.p(self.table_slots), self.table_cap, L.p(self.slab_base), self.slab_units,
                                                 self.res, self.voxel_length, self.sdf_trunc, L.p(out_d), L.p(out_v), L.p(out_n), L.p(out_c),
                                                 L.stream_ptr()), "bs_tsdf_raycast")
        pick = (lambda t: None if t is None else t[0]) if single else (lambda t: t)
        return RaycastFrame(pick(out_d), pick(out_c), pick(out_v), pick(out_n))

    # ---- views of the device state (tests, diagnostics) ---------------------------------------------
    @staticmethod
    def _np(m):
        return m.detach().cpu().numpy() if isinstance(m, torch.Tensor) else np.asarray(m)

    @property
    def index(self) -> list:
        """unit indices (ix, iy, iz) in block order"""
        return [tuple(int(v) for v in r) for r in self.unit_index[:self.n_units].cpu().numpy()]

    def unit(self, key) -> np.ndarray:
        """voxels of one unit as fp32 [res, res, res, 5]"""
        s = self.index.index(tuple(int(v) for v in key))
        return self.slabs[s // self.slab_units][s % self.slab_units].view(self.res, self.res, self.res, 5).cpu().numpy()


class MAP:
    """Drop-in for the reference's ``MAP`` (BodySLAM_not_refactored/3DM/tsdf.py:56-107), which wraps Open3D's tensor SLAM model
    (``o3d.t.pipelines.slam.Model(voxel_size, 16, block_count, ...)``): ``integrate(curr_rgbd, i, curr_global_pose)`` integrates
    a frame at its pose and then synthesises the model's view from that pose into ``raycast_frame`` (:81-83).

    Kept: the constructor and method names, blocks of 16^3 voxels, ``block_count`` as the map's capacity, truncation =
    ``trunc_voxel_multiplier * voxel_size``, and a synthesised frame (depth + colour, a ``RaycastFrame``) after every
    integration, cast between the frame's ``depth_min`` and ``depth_max``.  Not kept: Open3D's tensor integration weights (the
    voxels are this package's ``TSDF`` running means, csrc/tsdf.hip); its frame-pose bookkeeping (``update_frame_pose``) is the
    list ``frame_poses``.  ``curr_global_pose`` is the camera -> world 4x4 (Open3D's T_frame_to_model).  ``curr_rgbd`` is this
    package's ``RGBDImage`` (depth in metres; an integer depth image is divided by ``depth_scale``) or any object with ``color``
    and ``depth``; its ``depth_min`` / ``depth_max`` attributes (metres) are used when present, as the reference reads them from
    its frame, otherwise the minimum and maximum of the depth image -- one read-back per frame.  The rays start ``sdf_trunc``
    before ``depth_min`` and run ``sdf_trunc`` past ``depth_max``: a surface is found where the tsdf changes sign, between a
    sample in front of it and one behind it, so the nearest and the farthest pixel of the frame need that margin."""

    def __init__(self, width, height, intrinsic, device, depth_scale, voxel_size=0.0058, block_count=40000, trunc_voxel_multiplier=8.0):
        if not isinstance(intrinsic, PinholeCameraIntrinsic):
            m = np.asarray(TSDF._np(intrinsic), dtype=np.float64)          # Open3D's Frame takes the 3x3 matrix
            intrinsic = PinholeCameraIntrinsic(int(width), int(height), float(m[0, 0]), float(m[1, 1]), float(m[0, 2]), float(m[1, 2]))
        self.intrinsic = intrinsic
        self.width, self.height = int(width), int(height)
        self.depth_scale, self.trunc_voxel_multiplier = float(depth_scale), float(trunc_voxel_multiplier)
        index = device if isinstance(device, int) else (torch.device(device).index or 0)
        self.model = TSDF(float(voxel_size), self.trunc_voxel_multiplier * float(voxel_size), volume_unit_resolution=16, device=index,
                          max_units=int(block_count))
        self.frame_poses = []                                               # (i, camera -> world) per integrate call
        self.raycast_frame: Optional[RaycastFrame] = None
        self.last_tracking: Optional[TrackingResult] = None                 # of the last track_frame_to_model call
        self._tracker = None                                                # ((iterations, depth_diff), PointToPlaneOdometry)

    def _depth_m(self, depth) -> torch.Tensor:
        """a frame's depth as fp32 metres on the device: an integer depth image is divided by ``depth_scale``"""
        if isinstance(depth, torch.Tensor):
            depth = depth.to(self.model.dev)
            return depth.to(torch.float32) if depth.is_floating_point() else depth.to(torch.float32) / self.depth_scale
        depth = np.asarray(depth)
        depth = depth.astype(np.float32) if depth.dtype.kind == "f" else depth.astype(np.float32) / np.float32(self.depth_scale)
        return torch.from_numpy(np.ascontiguousarray(depth)).to(self.model.dev)

    def integrate(self, curr_rgbd, i, curr_global_pose) -> None:
        depth = self._depth_m(curr_rgbd.depth)
        pose = np.asarray(TSDF._np(curr_global_pose), dtype=np.float64)
        E = np.linalg.inv(pose)
        self.frame_poses.append((i, pose))
        self.model.build_3D_map(RGBDImage(curr_rgbd.color, depth), self.intrinsic, E)
        lo, hi = getattr(curr_rgbd, "depth_min", None), getattr(curr_rgbd, "depth_max", None)
        if lo is None or hi is None:
            lo, hi = (float(v) for v in torch.stack([depth.min(), depth.max()]).cpu())
        lo, hi = max(float(lo) - self.model.sdf_trunc, 0.0), float(hi) + self.model.sdf_trunc
        self.raycast_frame = self.model.raycast(self.intrinsic, E, depth_min=lo, depth_max=hi, color=True)

    def track_frame_to_model(self, curr_rgbd, depth_max: Optional[float] = None, depth_diff: float = 0.07, iterations: Sequence[int] = (6, 3, 1),
                             init=None) -> TrackingResult:
        """Where ``curr_rgbd`` sits relative to the map: its depth is registered against ``raycast_frame.depth`` (the model as the
        last integrated pose sees it) by point-to-plane odometry -- the role of Open3D's ``Model.track_frame_to_model(input_frame,
        raycast_frame, depth_scale, depth_max=3.0, depth_diff=0.07)``; parity with Open3D unpinned, the algorithm is
        ``rgbd_odometry.PointToPlaneOdometry``'s.  Depth conventions as in ``integrate``; depth_max: the frame's ``depth_max``
        attribute when it has one, else 3.0 m.  init: a first guess of the transformation (default: the identity)."""
        if self.raycast_frame is None:
            raise RuntimeError("MAP.track_frame_to_model: the map has no raycast_frame yet -- integrate a frame first")
        from .rgbd_odometry import PointToPlaneOdometry
        key = (tuple(int(v) for v in iterations), float(depth_diff))
        if self._tracker is None or self._tracker[0] != key:
            K = (self.intrinsic.fx, self.intrinsic.fy, self.intrinsic.cx, self.intrinsic.cy)
            self._tracker = (key, PointToPlaneOdometry(K, device=self.model.dev.index or 0, iterations=key[0], depth_diff=key[1]))
        odo = self._tracker[1]
        if depth_max is None:
            depth_max = getattr(curr_rgbd, "depth_max", None)
        depth = self._depth_m(curr_rgbd.depth)
        T = np.eye(4)
        T[:3] = odo.estimate_batch(depth[None], self.raycast_frame.depth[None], init=init,
                                   depth_max=3.0 if depth_max is None else float(depth_max)).cpu().numpy().reshape(3, 4)
        sums = odo.last_sums[0].cpu().numpy()             # the last step's: at the finest level, at the pose before its update
        inliers = int(round(sums[28]))
        self.last_tracking = TrackingResult(T, self.frame_poses[-1][1] @ T, inliers, float(sums[27]), inliers / float(depth.shape[0] * depth.shape[1]))
        return self.last_tracking

    def track_and_integrate(self, curr_rgbd, i, init=None) -> np.ndarray:
        """Track the frame against the map, then integrate it at the tracked pose; returns that pose (camera -> world).  init: a
        first guess of the frame's pose.  On an empty map there is nothing to track against: the frame is integrated at ``init``,
        or at the identity."""
        guess = None if init is None else np.asarray(TSDF._np(init), dtype=np.float64)
        if self.raycast_frame is None:
            pose = np.eye(4) if guess is None else guess
        else:
            pose = self.track_frame_to_model(curr_rgbd, init=None if guess is None else np.linalg.inv(self.frame_poses[-1][1]) @ guess).pose
        self.integrate(curr_rgbd, i, pose)
        return pose

    def extract_pcd(self, host: bool = True) -> PointCloud:
        return self.model.extract_pcd(host=host)

    def extract_mesh(self, host: bool = True) -> TriangleMesh:
        return self.model.extract_mesh(host=host)

    def save_pcd(self, saving_path: str) -> None:
        self.model.save_pcd(saving_path)

    def save_mesh(self, saving_path: str) -> None:
        self.model.save_mesh(saving_path)


def write_ply(path: str, pcd: PointCloud) -> None:
    """binary little-endian PLY: x y z (float32) [nx ny nz (float32)] red green blue (uchar) -- the container o3d.io.write_point_cloud
    produces for a .ply path (Open3D stores coordinates and normals as doubles; the values here are fp32)"""
    n = pcd.points.shape[0]
    has_n = pcd.normals is not None
    fields = [("x", "<f4"), ("y", "<f4"), ("z", "<f4")] + ([("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4")] if has_n else []) + \
             [("red", "u1"), ("green", "u1"), ("blue", "u1")]
    rec = np.empty(n, dtype=fields)
    rec["x"], rec["y"], rec["z"] = pcd.points[:, 0], pcd.points[:, 1], pcd.points[:, 2]
    if has_n:
        rec["nx"], rec["ny"], rec["nz"] = pcd.normals[:, 0], pcd.normals[:, 1], pcd.normals[:, 2]
    c = np.clip(np.rint(pcd.colors * 255.0), 0, 255).astype(np.uint8) if n else np.zeros((0, 3), np.uint8)
    rec["red"], rec["green"], rec["blue"] = c[:, 0], c[:, 1], c[:, 2]
    props = "property float x\nproperty float y\nproperty float z\n" + ("property float nx\nproperty float ny\nproperty float nz\n" if has_n else "")
    with open(path, "wb") as f:
        f.write((f"ply\nformat binary_little_endian 1.0\ncomment bodyslam_amd TSDF point cloud\nelement vertex {n}\n" + props +
                 "property uchar red\nproperty uchar green\nproperty uchar blue\nend_header\n").encode("ascii"))
        f.write(rec.tobytes())


def write_ply_mesh(path: str, mesh: TriangleMesh) -> None:
    """binary little-endian PLY of a triangle mesh: vertices x y z (float32) red green blue (uchar), faces as uchar-counted int32 lists
    -- what o3d.io.write_triangle_mesh writes for a .ply path (Open3D stores coordinates as doubles; the values here are fp32)"""
    nv, nt = mesh.vertices.shape[0], mesh.triangles.shape[0]
    vrec = np.empty(nv, dtype=[("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("red", "u1"), ("green", "u1"), ("blue", "u1")])
    vrec["x"], vrec["y"], vrec["z"] = mesh.vertices[:, 0], mesh.vertices[:, 1], mesh.vertices[:, 2]
    c = np.clip(np.rint(mesh.vertex_colors * 255.0), 0, 255).astype(np.uint8) if nv else np.zeros((0, 3), np.uint8)
    vrec["red"], vrec["green"], vrec["blue"] = c[:, 0], c[:, 1], c[:, 2]
    frec = np.empty(nt, dtype=[("n", "u1"), ("a", "<i4"), ("b", "<i4"), ("c", "<i4")])
    frec["n"] = 3
    if nt:
        frec["a"], frec["b"], frec["c"] = mesh.triangles[:, 0], mesh.triangles[:, 1], mesh.triangles[:, 2]
    with open(path, "wb") as f:
        f.write((f"ply\nformat binary_little_endian 1.0\ncomment bodyslam_amd TSDF triangle mesh\nelement vertex {nv}\n"
                 "property float x\nproperty float y\nproperty float z\nproperty uchar red\nproperty uchar green\nproperty uchar blue\n"
                 f"element face {nt}\nproperty list uchar int vertex_indices\nend_header\n").encode("ascii"))
        f.write(vrec.tobytes())
        f.write(frec.tobytes())
