"""Time TSDF.raycast (bs_tsdf_raycast) at the reference's map parameters (1 mm voxels, 0.1 m truncation, 32^3 units, stride 8):
a synthetic RGB-D sequence -- 64 views of a textured height field at ~0.3 m along a smooth camera path, rendered on the device --
is integrated with build_3D_map_batch, then the model is ray-cast at 640x480, one view per call and 64 views per call, beside
extract_pcd of the same map (the only other way the package has to read the surface back).

    python tools/raycast_time.py [--frames 64] [--height 480] [--width 640] [--reps 10] [--json PATH]

Device events around each call after a warm-up, median of the repetitions; extract_pcd ends on the host and is timed with the host
clock around it.  Reports ms per view and rays/s for depth + colour (the default outputs) and for all four outputs, and the
accuracy of the first view against the renderer.  Kernel times: run this under `rocprofv3 --kernel-trace --stats` in a run of its
own (--reps 3 is enough there).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def pose_of(i, n):
    """camera -> world of view i: a slow arc over the surface (a few centimetres and degrees over the sequence)"""
    s = i / max(n - 1, 1)
    rx, ry, rz = 0.06 * np.sin(2.0 * np.pi * s), -0.08 * s + 0.04, 0.03 * s
    cx, sx, cy, sy, cz, sz = np.cos(rx), np.sin(rx), np.cos(ry), np.sin(ry), np.cos(rz), np.sin(rz)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    T = np.eye(4)
    T[:3, :3] = Rz @ Ry @ Rx
    T[:3, 3] = (0.03 * s - 0.015, 0.02 * np.sin(np.pi * s), 0.01 * s)
    return T


def render(torch, pose, K, H, W, dev):
    """depth fp32 [H, W] (camera-frame z) and colour u8 [H, W, 3] of the height field Z = g(X, Y), by Newton iterations per ray"""
    def g(X, Y):
        return 0.30 + 0.03 * torch.sin(9.0 * X) * torch.cos(7.0 * Y) + 0.02 * torch.cos(5.0 * X + 3.0 * Y)
    fx, fy, cx, cy = K
    v, u = torch.meshgrid(torch.arange(H, device=dev, dtype=torch.float64), torch.arange(W, device=dev, dtype=torch.float64), indexing="ij")
    dc = torch.stack([(u - cx) / fx, (v - cy) / fy, torch.ones_like(u)], -1)
    P = torch.from_numpy(pose).to(dev)
    d, o = dc @ P[:3, :3].T, P[:3, 3]
    s = torch.full((H, W), 0.3, device=dev, dtype=torch.float64)
    eps = 1e-6
    for _ in range(20):
        X = o + s[..., None] * d
        F = X[..., 2] - g(X[..., 0], X[..., 1])
        gx = (g(X[..., 0] + eps, X[..., 1]) - g(X[..., 0] - eps, X[..., 1])) / (2 * eps)
        gy = (g(X[..., 0], X[..., 1] + eps) - g(X[..., 0], X[..., 1] - eps)) / (2 * eps)
        s = s - F / (d[..., 2] - gx * d[..., 0] - gy * d[..., 1])
    X = o + s[..., None] * d
    tex = lambda a, b, c: 0.5 + 0.25 * torch.sin(a * X[..., 0] + c) * torch.cos(b * X[..., 1] - c) + 0.2 * torch.sin((a + b) * (X[..., 0] - X[..., 1]) + 2 * c)
    col = torch.stack([tex(60, 45, 0.3), tex(40, 70, 1.1), tex(75, 30, 2.0)], -1)
    return s.to(torch.float32), torch.clamp(torch.round(col * 255.0), 0, 255).to(torch.uint8)


def median_ms(torch, fn, reps):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    fn()                                                                    # warm-up (code object, allocator)
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        ev[0].record()
        fn()
        ev[1].record()
        ev[1].synchronize()
        ms.append(ev[0].elapsed_time(ev[1]))
    ms.sort()
    return ms[len(ms) // 2], ms[0]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    import torch
    from bodyslam_amd import _lib as L
    from bodyslam_amd.tsdf import TSDF, PinholeCameraIntrinsic, RGBDImage
    L.init(0)
    dev = torch.device("cuda:0")
    N, H, W = a.frames, a.height, a.width
    K = (600.0 * W / 640.0, 600.0 * W / 640.0, W / 2.0, H / 2.0)
    intr = PinholeCameraIntrinsic(W, H, *K)
    poses = [pose_of(i, N) for i in range(N)]
    E = np.stack([np.linalg.inv(P) for P in poses])
    frames = [render(torch, P, K, H, W, dev) for P in poses]
    tsdf = TSDF()
    t0 = time.perf_counter()
    tsdf.build_3D_map_batch([RGBDImage(c, d) for d, c in frames], intr, list(E))
    tsdf.sync()
    torch.cuda.synchronize()
    build_ms = (time.perf_counter() - t0) * 1e3
    voxel_bytes = tsdf.n_units * tsdf.unit_floats * 4
    res = {"frames": N, "height": H, "width": W, "units": tsdf.n_units, "voxel_store_bytes": voxel_bytes, "build_ms_wall": build_ms}
    print(f"map: {N} frames of {W}x{H} -> {tsdf.n_units} units = {voxel_bytes / 1e9:.2f} GB of voxel state (built in {build_ms:.0f} ms wall, "
          f"allocation included)")
    kw = dict(depth_min=0.05, depth_max=1.0)
    # accuracy of what is timed: view 0 against the renderer
    got = tsdf.raycast(intr, E[0], **kw).depth
    hit = got > 0
    err = (got - frames[0][0]).abs()[hit] / tsdf.voxel_length
    res["view0"] = {"hit_share": float(hit.float().mean()), "median_err_voxels": float(err.median()), "max_err_voxels": float(err.max())}
    print(f"view 0: hit share {res['view0']['hit_share']:.4f}, |depth - truth| median {res['view0']['median_err_voxels']:.3f} max "
          f"{res['view0']['max_err_voxels']:.3f} voxels")
    for nv in (1, N):
        Ev = E[0] if nv == 1 else E
        for name, extra in (("depth+colour", {}), ("all outputs", dict(vertex=True, normal=True))):
            med, best = median_ms(torch, lambda: tsdf.raycast(intr, Ev, **kw, **extra), a.reps)
            r = {"ms_per_call": med, "ms_per_call_min": best, "ms_per_view": med / nv, "rays_per_s": nv * H * W / (med * 1e-3)}
            res[f"{nv}_views_{name.replace(' ', '_')}"] = r
            print(f"raycast {nv:3d} view(s), {name:12s}: {med:8.3f} ms per call (min {best:.3f}) = {r['ms_per_view']:.3f} ms per view, "
                  f"{r['rays_per_s'] / 1e9:.2f} G rays/s")
    ex = []
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        pcd = tsdf.extract_pcd()
        ex.append((time.perf_counter() - t0) * 1e3)
    ex.sort()
    res["extract_pcd"] = {"ms_wall": ex[1], "points": int(pcd.points.shape[0])}
    print(f"extract_pcd: {ex[1]:.1f} ms wall (host copy of {pcd.points.shape[0]} points included; its two kernels stream the voxel store twice: "
          f"{2 * voxel_bytes / 1e9:.2f} GB)")
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
