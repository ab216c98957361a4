"""Time bodyslam_amd.evaluation.evaluate_depth (bs_depth_metrics) on a long sequence: 2 560 frames of 640x480 by default, the size the
benchmark's sequence produces, as device tensors (the depth_u16 of a SequenceResult stays in HBM).

    python tools/depth_eval_time.py [--frames 2560] [--height 480] [--width 640] [--reps 10] [--json PATH]

Device events around each call after a warm-up; two inputs: a spread one (smooth Hamlyn-like GT in mm, smooth prediction) and a skewed
one (every frame constant: every histogram atomic of a frame lands on one bin).  Reports ms per sequence, frames/s and the bytes
rate against one read of both maps (B*H*W*4 bytes) and three reads (the two histogram passes and the metrics pass).  Kernel times:
run this under `rocprofv3 --kernel-trace --stats` in a run of its own.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def make_inputs(torch, B, H, W, skewed, dev):
    g = torch.Generator(device=dev).manual_seed(1)
    if skewed:
        gt = torch.full((B, H, W), 150, dtype=torch.int16, device=dev)
        pred = torch.full((B, H, W), 700, dtype=torch.int16, device=dev)
        return pred, gt
    y = torch.linspace(0, 1, H, device=dev)[:, None]
    x = torch.linspace(0, 1, W, device=dev)[None, :]
    ph = torch.rand(B, 1, 1, generator=g, device=dev) * 6.3
    base = 0.5 + 0.3 * torch.sin(4 * x + ph) * torch.cos(3 * y + ph) + 0.05 * torch.rand(B, H, W, generator=g, device=dev)
    gt = (base * 400).clamp(0, 65535).to(torch.int32).to(torch.int16)
    pred = (base.flip(-1) * 3000 + 100).clamp(0, 65535).to(torch.int32).to(torch.int16)
    return pred, gt


def time_case(torch, E, L, pred, gt, reps):
    B, H, W = pred.shape
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
    E.evaluate_depth(pred, gt, "hamlyn")                                   # warm-up (code objects, allocator)
    call = []
    for _ in range(reps):
        ev[0].record()
        E.evaluate_depth(pred, gt, "hamlyn")
        ev[1].record()
        ev[1].synchronize()
        call.append(ev[0].elapsed_time(ev[1]))
    # the launches alone: preallocated workspace and output, no host copy
    ws = torch.empty(L.depth_metrics_workspace(B, H, W), dtype=torch.uint8, device=pred.device)
    out = torch.empty(B, L.DEPTH_METRICS_FIELDS, dtype=torch.float64, device=pred.device)
    L.depth_metrics(pred, gt, 1.0, 300.0, None, ws, out)
    torch.cuda.synchronize()
    launch = []
    for _ in range(reps):
        ev[2].record()
        L.depth_metrics(pred, gt, 1.0, 300.0, None, ws, out)
        ev[3].record()
        ev[3].synchronize()
        launch.append(ev[2].elapsed_time(ev[3]))
    call.sort()
    launch.sort()
    return call[len(call) // 2], launch[len(launch) // 2], min(launch)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--frames", type=int, default=2560)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    import torch
    from bodyslam_amd import _lib as L
    from bodyslam_amd import evaluation as E
    L.init(0)
    dev = torch.device("cuda:0")
    B, H, W = a.frames, a.height, a.width
    one_read = B * H * W * 4
    res = {"frames": B, "height": H, "width": W, "one_read_bytes": one_read, "three_read_bytes": 3 * one_read}
    for name, skewed in (("spread", False), ("constant", True)):
        pred, gt = make_inputs(torch, B, H, W, skewed, dev)
        call_ms, launch_ms, launch_min = time_case(torch, E, L, pred, gt, a.reps)
        r = {"evaluate_depth_ms": call_ms, "launches_ms": launch_ms, "launches_min_ms": launch_min,
             "frames_per_s": B / (call_ms * 1e-3), "one_read_GBps": one_read / (launch_ms * 1e-3) / 1e9,
             "three_read_GBps": 3 * one_read / (launch_ms * 1e-3) / 1e9}
        res[name] = r
        print(f"{name:8s} {B} x {H}x{W}: evaluate_depth {call_ms:.3f} ms ({r['frames_per_s']:.0f} frames/s); launches {launch_ms:.3f} ms "
              f"(min {launch_min:.3f}) = {r['one_read_GBps']:.0f} GB/s of one read, {r['three_read_GBps']:.0f} GB/s of three")
        del pred, gt
        torch.cuda.empty_cache()
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
