"""Probe: the TSDF map at the reference's own parameters (1 mm voxels, 0.1 m truncation, 32^3 units, stride 8; 3DM/tsdf.py:6-12)
on 640x480 frames resident on the device -- units touched and opened per frame, the time of a synchronous build_3D_map call (HIP
events around it: upload of the record, unit discovery, the round trip that makes the blocks, assignment and integration) and the
HBM rate that is of the touched voxel state, extraction time."""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from bodyslam_amd.tsdf import TSDF, PinholeCameraIntrinsic, RGBDImage   # noqa: E402

H, W = 480, 640
K = (383.1901395, 383.1901395, 276.4727783203125, 124.3335933685303)          # slam.py:25-28
v, u = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
rng = np.random.default_rng(0)
color = torch.from_numpy(rng.integers(0, 256, size=(H, W, 3)).astype(np.uint8)).cuda()
intr = PinholeCameraIntrinsic(W, H, *K)
t = TSDF()
ms = []
for f in range(int(sys.argv[1]) if len(sys.argv) > 1 else 3):
    depth = torch.from_numpy((0.12 + 0.03 * np.sin(u / 90.0 + 0.3 * f) * np.cos(v / 70.0)).astype(np.float32)).cuda()   # an endoscopic working distance
    pose = np.eye(4)
    pose[:3, 3] = (0.002 * f, 0.0, 0.001 * f)
    E = np.linalg.inv(pose)
    n0 = t.n_units
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    torch.cuda.synchronize()
    tw = time.perf_counter()
    ev[0].record()
    t.build_3D_map(RGBDImage(color, depth), intr, E)
    ev[1].record()
    t1 = time.perf_counter()
    ev[1].synchronize()
    n_units, touched = t.sync()
    nv = touched * 32 ** 3
    ms.append(ev[0].elapsed_time(ev[1]))
    print(f"frame {f}: {touched} units touched ({n_units - n0} new), {nv / 1e6:.0f} M voxels = {nv * 20 / 1e9:.2f} GB of voxel state; build_3D_map "
          f"{ms[-1]:.3f} ms (HIP events; upper bound of the integration's traffic, 40 B x every voxel of the touched units: "
          f"{nv * 40 / (ms[-1] * 1e-3) / 1e12:.2f} TB/s), host side of the call {(t1 - tw) * 1e3:.2f} ms", flush=True)
if len(ms) > 2:
    print(f"build_3D_map, frames 2 onwards: median {float(np.median(ms[2:])):.3f} ms, min {min(ms[2:]):.3f} ms")
t0 = time.perf_counter()
pcd = t.extract_pcd()
torch.cuda.synchronize()
print(f"extract_pcd: {pcd.points.shape[0]} points from {len(t.index)} units in {(time.perf_counter() - t0) * 1e3:.0f} ms; "
      f"allocated {torch.cuda.memory_allocated() / 1e9:.1f} GB")
