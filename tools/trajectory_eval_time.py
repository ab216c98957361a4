"""Times the trajectory evaluation on the device: bs_trajectory_metrics at S = 256 x N = 1000 and S = 1 x N = 4000 (both protocols), the
numpy restatement tests/_trajectory_eval_ref.py on the same machine's CPU, and bs_similarity_fit at 1 000 (launch latency), 2 M and 20 M
points with the achieved HBM bandwidth (two passes over both point sets).  HIP events, median of 10 after warm-up.  Reported, not asserted.

    python tools/trajectory_eval_time.py [--out profiles/trajectory_eval_time.txt]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _trajectory_eval_ref as TR  # noqa: E402
from bodyslam_amd import _lib as L  # noqa: E402

HBM_ACHIEVABLE_TBS = 6.3


def gpu_median_ms(fn, reps=10, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "trajectory_eval_time.txt"))
    a = ap.parse_args()
    L.init(0)
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    lines = [f"trajectory evaluation timing on {torch.cuda.get_device_name(0)} (HIP events, median of 10, warmed)"]
    flags = L.TRAJ_ALIGN_ORIGIN | L.TRAJ_ALIGN | L.TRAJ_CORRECT_SCALE
    gt1 = TR.random_walk(rng, 4000)
    pr1 = TR.perturbed(rng, gt1)
    for S, N in ((256, 1000), (1, 4000)):
        g = np.tile(gt1[:N], (S, 1, 1))
        p = np.tile(pr1[:N], (S, 1, 1))
        gd, pd = torch.from_numpy(g).to(dev).reshape(-1, 16), torch.from_numpy(p).to(dev).reshape(-1, 16)
        off = torch.arange(0, (S + 1) * N, N, dtype=torch.int32, device=dev)
        out = torch.empty(S, L.TRAJ_FIELDS, dtype=torch.float64, device=dev)
        for pname, proto in (("evo", L.TRAJ_EVO), ("training", L.TRAJ_TRAINING)):
            ms = gpu_median_ms(lambda: L.trajectory_metrics(gd, pd, off, proto, 1, flags, out))
            t0 = time.perf_counter()
            TR.evaluate(gt1[:N], pr1[:N], protocol=pname)
            cpu_ms = (time.perf_counter() - t0) * 1e3
            lines.append(f"bs_trajectory_metrics {pname:8s} S={S:4d} N={N:5d}: {ms:8.3f} ms on the device; numpy restatement, one sequence "
                         f"{cpu_ms:8.1f} ms -> {cpu_ms * S:10.1f} ms for the batch on the CPU")
    ws = torch.empty(L.SIMILARITY_FIT_WORKSPACE_BYTES, dtype=torch.uint8, device=dev)
    out = torch.empty(16, dtype=torch.float64, device=dev)
    for n in (1_000, 2_000_000, 20_000_000):          # n = 1 000: the latency of the four launches and the serial finish, no bandwidth to speak of
        for dt in (torch.float32, torch.float64):
            x = torch.randn(n, 3, device=dev, dtype=dt)
            y = (1.5 * x + 0.25).contiguous()
            ms = gpu_median_ms(lambda: L.similarity_fit(x, y, ws, out))
            nbytes = 2 * 2 * n * 3 * x.element_size()
            tbs = nbytes / (ms * 1e-3) / 1e12
            line = (f"bs_similarity_fit {str(dt).split('.')[-1]:8s} n={n:9d}: {ms:8.3f} ms, {nbytes / 1e6:8.1f} MB read, {tbs:5.2f} TB/s "
                    f"({100 * tbs / HBM_ACHIEVABLE_TBS:4.1f} % of {HBM_ACHIEVABLE_TBS} TB/s)")
            if dt == torch.float32 and n == 2_000_000:
                xh, yh = x.cpu().numpy().astype(np.float64), y.cpu().numpy().astype(np.float64)
                t0 = time.perf_counter()
                TR.umeyama(xh, yh)
                line += f"; numpy restatement {(time.perf_counter() - t0) * 1e3:.1f} ms"
            lines.append(line)
            del x, y
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
