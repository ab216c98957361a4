#!/usr/bin/env python3
"""Benchmark of the BodySLAM hot path on MI355X: frames/s of depth (ZoeD_NK, flip-aug) + relative pose
(CyclePose) + pose chain + back-projection on synthetic 640x480 sequences.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--batch B] [--dtype f16|bf16] [--precision accurate|fast]
                    [--full] [--dump-outputs DIR]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \
        bench.py --gpus N --steps K --warmup W

A plain run (no --full) does only what the headline needs: set-up (weights, frames, pipeline, calibration), W warm-up steps, K timed
steps of --precision, the result line (`metric`, `value`, `unit`, `higher_is_better`, `dtype`, `ms_per_step`, ...).  Its frames are
made on the device (device_sequence: make_sequence_at's construction, noise from a seeded device generator), so set-up does not grow
with K.  --full adds everything else described below, as before: the other precision mode, the CPU baseline and the depth check
against the oracle (frames made on the host by make_sequence, before the first GPU call), per-kernel HIP-event timing and the
rooflines, the PMC traffic child runs, board power, and the PCIe, outlier-weights, SLAM-loop and latency legs; the --no-* switches
below select among them.
--dump-outputs DIR: after the timed steps, what the last timed step computed -- the arrays its caller receives (depth maps, relative
and absolute poses, point counts, back-projected points; the per-frame arrays for a fixed, seeded sample of the batch's frames, < 64 MB
in all) -- goes to DIR/<name>.npy in float32 / float64 (rank 0's block at N > 1).  The same arguments give the same inputs.

A step = one pass of the full loop over one batch of B consecutive frames per rank (default B = 128, 2 steps = 256 frames):
  MDEM  B frames -> 2B network forwards (flip-aug) -> B depth maps (fp32 metres + uint16)
  MPEM  the B frame pairs (i-1, i) of the batch (one halo frame) -> B relative poses
  RCCL  all-gather of the per-rank [B,16] relatives (N > 1), fp64 pose chain over the gathered block
  3DM   back-projection + compaction of the rank's B depth maps with their absolute poses
Inputs are resident in HBM before the timed region.  K steps are timed between barrier +
torch.cuda.synchronize() pairs; the value is (ranks x K x B frames) / max-over-ranks time.
Weights are random-init (no checkpoint is reachable offline); data is synthetic.  The chain continues from step to step
(bs_pose_chain_from: the last absolute pose of a step is the next step's g0, on the device).  At N > 1 (weak scaling: B frames per
rank and step) the ranks process ONE sequence: step k hands rank r the B frames that follow rank r - 1's block, with that block's
last frame as its halo, so the gathered world x B relatives of a step are consecutive poses of the same sequence (BASELINE config
4's semantics at a fixed per-GPU load); every rank synthesises only the frames it owns (synthetic.make_sequence_at).

--scaling strong: ONE sequence of --frames frames (default 1000: BASELINE config 4) is cut into contiguous blocks by
shard_bounds (ragged: 125 frames per rank at 8 GPUs); a step = BodySlamPipeline.run_sequence over the whole sequence
(every rank: depth + pose on its block with the one-frame halo, ONE all-gather of the relatives, the replicated fp64
chain, back-projection of its block); value = K x frames / max-over-ranks time; "scaling": "strong".

The primary line is precision="accurate" (split-precision products, depth L1 vs the fp32 oracle <= 1e-4 m -- the north
star's tolerance); with --full the single-pass "fast" mode is measured in the same run and reported under "other_mode".

roofline: per-kernel HIP-event timing of every bs_gemm launch inside the timed steps, aggregated per
kernel instantiation (tile variant x conv/plain); the dominant one by time is reported against the dense
fp16/bf16 MFMA peak (2.5 PFLOP/s), next to the conv-stack aggregate the north star names.  `achieved` counts algorithmic
FLOPs (2*M*N*K of the product computed), `executed` the MFMA work issued in 16-bit-equivalents (2x in accurate mode).
cpu_baseline: the CPU oracle (torch fp32, up to 32 host threads) on EIGHT frames of the same workload, rank 0 only, taken BEFORE this
process touches the GPU (round 6: after the GPU legs it read 0.19-0.55 frames/s depending on what had run).  The same eight oracle depth
maps are the yardstick of `depth_l1_frames`: eight frames spread over the timed steps, copied out of the timed plan's output.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

MFMA_PEAK_TFLOPS = 2500.0   # dense fp16/bf16, /opt/skills/guides/MI355X_MICROARCH.md "Chip-level parameters"
CONV_STACK_GFLOP_PER_FORWARD = 233.6   # neck + relative head + metric head + patch-embed convolutions of ONE ZoeD_NK forward
                                       # at 384x512 (2 x MACs of the reference's own formulation); scales with the network input's pixels
N_CHECK_FRAMES = 8                     # frames of the timed steps compared with the CPU oracle (depth_l1_frames)
TILE_NAMES = {1: "128x128x64s2", 2: "128x64x64s2", 3: "128x32x64s2", 9: "256x256x64s2", 10: "256x256x32s4pp", 11: "256x128x32s3"}   # csrc/igemm.hip


def measure_pmc_traffic(args):
    """{kernel name: (launches, mean FETCH_SIZE KB, mean WRITE_SIZE KB)} from two `rocprofv3 --pmc` child runs, or None."""
    import csv
    import shutil
    import subprocess
    import tempfile
    exe = shutil.which("rocprofv3") or ("/opt/rocm/bin/rocprofv3" if os.path.exists("/opt/rocm/bin/rocprofv3") else None)
    if exe is None:
        return None
    out = {}
    tmp = tempfile.mkdtemp(prefix="bs_pmc_", dir="/tmp")
    env = dict(os.environ, TMPDIR="/tmp")
    try:
        for counter in ("FETCH_SIZE", "WRITE_SIZE"):
            cmd = [exe, "--kernel-trace", "--pmc", counter, "--output-format", "csv", "-d", tmp, "-o", counter, "--",
                   "python3", os.path.join(ROOT, "bench.py"), "--full", "--single-mode", "--precision", args.precision, "--steps", "1", "--warmup", "0",
                   "--batch", str(args.batch), "--dtype", args.dtype, "--height", str(args.height), "--width", str(args.width),
                   "--weights", args.weights, "--weights-seed", str(args.weights_seed), "--no-cpu-baseline", "--no-kernel-timing", "--no-pmc-traffic", "--no-slam-loop", "--no-outlier-leg",
                   "--no-pcie-leg", "--no-latency-leg"]
            subprocess.run(cmd, cwd="/tmp", env=env, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=240, check=True)
            path = None
            for dp, _, fns in os.walk(tmp):
                for fn in fns:
                    if fn.startswith(counter) and fn.endswith("counter_collection.csv"):
                        path = os.path.join(dp, fn)
            if path is None:
                return None
            with open(path, newline="") as f:
                for row in csv.DictReader(f):
                    if row["Counter_Name"] != counter:
                        continue
                    # per (kernel, grid size): the child also runs the calibration (~90 four-frame forwards) whose launches of the same
                    # instantiation are small -- the timed plan's launches are the ones with the kernel's LARGEST grid
                    key = (row["Kernel_Name"], int(row.get("Grid_Size") or row.get("Grid_Size_X") or 0))
                    a = out.setdefault(key, {"FETCH_SIZE": [0, 0.0], "WRITE_SIZE": [0, 0.0]})[counter]
                    a[0] += 1
                    a[1] += float(row["Counter_Value"])
        gmax, big = {}, {}
        for (name, grid) in out:
            gmax[name] = max(gmax.get(name, 0), grid)
        for (name, grid), v in out.items():
            if grid * 10 >= gmax[name]:          # the plan's launches: at least a tenth of the kernel's largest grid (the calibration's are 1 / 32 of the plan's)
                a = big.setdefault(name, {"FETCH_SIZE": [0, 0.0], "WRITE_SIZE": [0, 0.0]})
                for c_ in ("FETCH_SIZE", "WRITE_SIZE"):
                    a[c_][0] += v[c_][0]
                    a[c_][1] += v[c_][1]
        return {k: (max(v["FETCH_SIZE"][0], v["WRITE_SIZE"][0]), v["FETCH_SIZE"][1] / max(v["FETCH_SIZE"][0], 1),
                    v["WRITE_SIZE"][1] / max(v["WRITE_SIZE"][0], 1)) for k, v in big.items()}
    except Exception as e:      # no profiler / not permitted here: the line carries traffic = null
        print(f"[bench] PMC traffic pass skipped: {e!r}", file=sys.stderr)
        return None
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


class PowerSampler:
    """Board power and shader clock from the amdgpu hwmon files, sampled by a host thread every 25 ms over a timed region (no GPU call; best effort:
    `result()` is None where the files are not readable).  With several boards in sysfs the one drawing the most over the region is reported."""

    def __init__(self, pci: str = None):
        import glob
        self.nodes = [h for h in sorted(glob.glob("/sys/class/drm/card*/device/hwmon/hwmon*")) if self._rd(os.path.join(h, "name")) == "amdgpu"]
        # this process's board: the hwmon node under the PCI function torch reports for the device (a box shares its sysfs with the other tenants' GPUs)
        mine = [h for h in self.nodes if pci and os.path.realpath(os.path.join(h, "..", "..")).lower().endswith(pci.lower())]
        self.matched = bool(mine)
        if mine:
            self.nodes = mine
        self.rows = {h: [] for h in self.nodes}
        self._stop = False
        self._thread = None

    @staticmethod
    def _rd(path):
        try:
            with open(path) as f:
                return f.read().strip()
        except OSError:
            return None

    def _loop(self):
        while not self._stop:
            for h in self.nodes:
                pw = self._rd(os.path.join(h, "power1_average")) or self._rd(os.path.join(h, "power1_input"))
                fq = self._rd(os.path.join(h, "freq1_input"))
                if pw and pw.isdigit():
                    self.rows[h].append((float(pw) / 1e6, float(fq) / 1e6 if fq and fq.isdigit() else None))
            time.sleep(0.025)

    def start(self):
        if self.nodes:
            import threading
            self._thread = threading.Thread(target=self._loop, daemon=True)
            self._thread.start()
        return self

    def result(self):
        self._stop = True
        if self._thread is not None:
            self._thread.join()
        best = None
        for h, rows in self.rows.items():
            if len(rows) >= 4:
                pw = sorted(r[0] for r in rows)
                if best is None or pw[len(pw) // 2] > best[0]:
                    best = (pw[len(pw) // 2], h, rows)
        if best is None:
            return None
        med, h, rows = best
        fq = sorted(r[1] for r in rows if r[1] is not None)
        cap = self._rd(os.path.join(h, "power1_cap"))
        return {"median_w": round(med, 1), "max_w": round(max(r[0] for r in rows), 1), "cap_w": float(cap) / 1e6 if cap and cap.isdigit() else None,
                "sclk_mhz_median": round(fq[len(fq) // 2], 1) if fq else None, "samples": len(rows),
                "board": "the device's PCI function" if self.matched else "the board drawing the most (PCI function not matched)",
                "source": "amdgpu hwmon power1_average / freq1_input, 25 ms samples over the timed steps (host thread)"}


def device_sequence(n: int, h: int, w: int, seed: int, dev, chunk: int = 64) -> torch.Tensor:
    """[n, h, w, 3] uint8 frames of ONE synthetic sequence, made on `dev`: make_sequence_at's construction (the same eight sinusoids per
    channel drawn from `seed`, the field cropped along its diagonal, i.e. frame i shifted by i pixels, i.i.d. noise sigma = 8 around 106),
    with the noise drawn from a device generator seeded with `seed`.  The same arguments give the same frames; a plain run's set-up
    then costs milliseconds instead of ~17 ms of host time per frame."""
    rng = np.random.default_rng(seed)
    terms = [[] for _ in range(3)]
    for c in range(3):
        for _ in range(8):
            fy, fx = rng.uniform(0.002, 0.02, size=2)
            ph = rng.uniform(0, 2 * np.pi)
            amp = rng.uniform(5, 20)
            terms[c].append((float(fy), float(fx), float(ph), float(amp)))
    yy = np.arange(h + n, dtype=np.float64)[:, None]
    xx = np.arange(w + n, dtype=np.float64)[:, None]
    # amp sin(2 pi (fy y + fx x) + ph) = [amp sin(ay), amp cos(ay)] . [cos(bx), sin(bx)]: one [rows, 16] and one [cols, 16] table per channel
    ytab, xtab = [], []
    for c in range(3):
        fy, fx, ph, amp = (np.array([t[j] for t in terms[c]]) for j in range(4))
        ay = 2 * np.pi * fy[None, :] * yy + ph[None, :]
        bx = 2 * np.pi * fx[None, :] * xx
        ytab.append(torch.from_numpy(np.concatenate([np.sin(ay) * amp, np.cos(ay) * amp], 1).astype(np.float32)).to(dev))
        xtab.append(torch.from_numpy(np.concatenate([np.cos(bx), np.sin(bx)], 1).astype(np.float32)).to(dev))
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    out = torch.empty(n, h, w, 3, dtype=torch.uint8, device=dev)
    ar_h = torch.arange(h, device=dev)
    ar_w = torch.arange(w, device=dev)
    for i0 in range(0, n, chunk):
        i1 = min(n, i0 + chunk)
        fi = torch.arange(i0, i1, device=dev)
        rows, cols = fi[:, None] + ar_h[None, :], fi[:, None] + ar_w[None, :]
        fr = torch.randn(i1 - i0, h, w, 3, generator=g, device=dev).mul_(8.0).add_(106.0)
        for c in range(3):
            a, b = ytab[c][rows], xtab[c][cols]              # [f, h, 16], [f, w, 16]
            f_c = fr[..., c]
            for k in range(a.shape[-1]):
                f_c += a[:, :, k, None] * b[:, None, :, k]
        out[i0:i1] = fr.round_().clamp_(0, 255).to(torch.uint8)
    return out


def dump_outputs(path: str, last: dict, H: int, W: int):
    """The last timed step's outputs as float32 / float64 .npy files under `path`.  Per-frame arrays (depth maps, back-projected points)
    for a fixed, seeded sample of the step's frames, sized to stay below 64 MB in all; per-step arrays (poses, point counts) whole.
    points_xyz / points_idx: the first count entries of a frame are its points (backproject's layout), the rest NaN / -1."""
    os.makedirs(path, exist_ok=True)
    n = int(last["depth_u16"].shape[0])
    per_frame = H * W * 4 * (1 + 1 + 3 + 1)                 # depth_m, depth_u16, xyz, idx as float32
    n_sample = max(1, min(n, 8, (56 << 20) // per_frame))
    sample = np.sort(np.random.default_rng(0).choice(n, size=n_sample, replace=False))
    sel = torch.from_numpy(sample).to(last["depth_u16"].device)
    arrays = {}
    if last.get("depth_m") is not None:
        arrays["depth_m"] = last["depth_m"].index_select(0, sel).float().cpu().numpy()
    arrays["depth_u16"] = last["depth_u16"].index_select(0, sel).cpu().numpy().view(np.uint16).astype(np.float32)
    arrays["t_rel"] = last["t_rel"].float().cpu().numpy()
    arrays["g_abs"] = last["g_abs"].double().cpu().numpy()
    counts = last["counts"].cpu().numpy()
    arrays["point_counts"] = counts.astype(np.float64)
    if last.get("xyz") is not None:
        xyz = last["xyz"].index_select(0, sel).cpu().numpy().astype(np.float32)
        idx = last["idx"].index_select(0, sel).cpu().numpy().astype(np.float32)
        for r, j in enumerate(sample):
            xyz[r, counts[j]:] = np.nan
            idx[r, counts[j]:] = -1.0
        arrays["points_xyz"], arrays["points_idx"] = xyz, idx
    arrays["sample_frames"] = sample.astype(np.float64)       # which frames of the step the per-frame arrays hold
    for name, a in arrays.items():
        np.save(os.path.join(path, name + ".npy"), np.ascontiguousarray(a))


def weak_frame_indices(steps: int, B: int, world: int, rank: int):
    """N > 1, weak scaling: (frames of the ONE sequence, the indices rank `rank` holds).  Step k gives rank r the B frames
    (k * world + r) * B + 1 .. + B and, in front of them, the frame before (its halo = the last frame of rank r - 1's block of the same
    step, or of the last rank's block of step k - 1): `steps` x (B + 1) frames per rank, step k's at weak_chunk(k, B)"""
    total = steps * world * B + 1
    return total, [(k * world + rank) * B + j for k in range(steps) for j in range(B + 1)]


def weak_chunk(k: int, B: int) -> slice:
    return slice(k * (B + 1), (k + 1) * (B + 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--batch", type=int, default=128,
                    help="frames per step per GPU (2 steps x 128 = the 256-frame config; 256 network forwards per step).  128 since round 5: the 64-frame "
                         "step's GEMM grids are 6.02 rounds of the 256 CUs, the 128-frame step's 12.02 (+1.6 %% frames/s, 76 GB per plan)")
    ap.add_argument("--dtype", default="f16", choices=["f16", "bf16"])
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--precision", default="accurate", choices=["accurate", "fast", "reference"],
                    help="accurate: split-precision products, depth L1 <= 1e-4 m vs the fp32 oracle (the north star's tolerance); "
                         "fast: one 16-bit MFMA pass per product (L1 ~3e-4 m).  The other mode is measured too and reported beside it.  "
                         "reference: three 16-bit passes on (hi | lo) pairs per product (~1e-5 m): the mode in which bf16 storage meets the tolerance")
    ap.add_argument("--single-mode", action="store_true", help="measure only --precision")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-slam-loop", action="store_true", help="skip the extra `slam_loop` figure (the reference's whole per-frame loop around the hot path)")
    ap.add_argument("--no-kernel-timing", action="store_true", help="skip the per-launch HIP events (pure throughput run)")
    ap.add_argument("--scaling", default="weak", choices=["weak", "strong"],
                    help="weak: every rank runs its own sequence, --batch frames per step; strong: one --frames sequence cut across the ranks")
    ap.add_argument("--frames", type=int, default=1000, help="sequence length of --scaling strong (BASELINE config 4: 1000)")
    ap.add_argument("--weights", default="gaussian", choices=["gaussian", "outlier", "layerscale", "heavytail"],
                    help="statistics of the random-init ZoeDepth weights (bodyslam_amd.synthetic.WEIGHT_VARIANTS): 'outlier' = 6 channels 50x larger "
                         "behind every LayerNorm, what a trained BEiT carries -- the calibration then has to switch corrections back on")
    ap.add_argument("--weights-seed", type=int, default=0, help="seed of the random-init ZoeDepth weights (the headline is seed 0; tools/probes/seed_throughput.sh "
                                                                  "runs eight seeds: the calibration's choice, and with it the rate, depends on the weights)")
    ap.add_argument("--no-outlier-leg", action="store_true", help="skip the extra `outlier_weights` figure (the accurate mode on outlier-channel weights)")
    ap.add_argument("--no-pcie-leg", action="store_true", help="skip the extra `pcie_inclusive` figure (frames from pinned host memory, results copied back)")
    ap.add_argument("--no-latency-leg", action="store_true", help="skip the extra `latency_b1_ms` figures (one frame / one pair per call: the reference's call pattern)")
    ap.add_argument("--no-pmc-traffic", action="store_true",
                    help="skip the two rocprofv3 --pmc child runs (FETCH_SIZE, WRITE_SIZE) that measure roofline.traffic")
    ap.add_argument("--full", action="store_true",
                    help="measure everything beside the headline (other mode, CPU baseline + oracle depth check, kernel timing and rooflines, PMC "
                         "traffic, power, PCIe / outlier / SLAM-loop / latency legs); without it only --precision's timed steps run")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the last timed step's outputs to DIR/<name>.npy (float32 / float64, a seeded sample of the per-frame arrays)")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        sys.exit("bench.py: --steps must be >= 1 and --warmup >= 0")
    if not args.full:
        # the plain run: the headline's timed steps only (the --no-* switches all on, one precision mode)
        args.single_mode = True
        args.no_cpu_baseline = args.no_slam_loop = args.no_kernel_timing = args.no_pmc_traffic = True
        args.no_outlier_leg = args.no_pcie_leg = args.no_latency_leg = True

    if args.dtype == "bf16" and args.precision == "accurate":
        # BASELINE config 2 names bf16.  With e4m3 correction planes bf16 storage carries 8 + 4 significant bits -- fp16's single pass -- and
        # measures 1.3e-4 m: above the north star's 1e-4 m.  As (hi | lo) bf16 pairs with three MFMA passes per product (--precision
        # reference) it carries 16 bits and measures 1.3e-5 m (tests/test_zoedepth_gpu.py::test_bf16_reference_precision).  A bf16
        # "accurate" line would carry a tolerance it does not meet, so it is refused.
        sys.exit("bench.py: --dtype bf16 --precision accurate does not meet the 1e-4 m depth tolerance (1.3e-4 m).  bf16 meets it with "
                 "--precision reference (three 16-bit passes per product: 1.3e-5 m); the fastest tolerance-meeting configuration is --dtype f16 "
                 "(default).  Use --dtype bf16 --precision fast for a bf16 single-pass throughput line.")
    if args.precision == "reference":
        args.single_mode = True
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    # HBM traffic of every kernel by PMC counters, BEFORE this process touches the GPU: two child runs of this same command
    # (one timed step) under rocprofv3, FETCH_SIZE and WRITE_SIZE in separate passes as the microarch guide prescribes
    pmc = None
    if world == 1 and "RANK" not in os.environ and not args.no_pmc_traffic and args.scaling == "weak":
        pmc = measure_pmc_traffic(args)
    if world != args.gpus:
        if world == 1 and args.gpus > 1:
            sys.exit(f"--gpus {args.gpus} needs `python -m torch.distributed.run --nproc-per-node {args.gpus} bench.py ...`")
        args.gpus = world
    import torch.distributed as dist
    use_dist = world > 1 or "RANK" in os.environ        # under torch.distributed.run the RCCL path is exercised even at N=1

    from bodyslam_amd import _lib as L
    from bodyslam_amd import geom3d
    from bodyslam_amd.pipeline import BodySlamPipeline, gather_relative_poses
    from bodyslam_amd.synthetic import WEIGHT_VARIANTS, make_sequence, random_cyclepose_weights, random_zoedepth_weights
    from bodyslam_amd.zoedepth import ZoeConfig

    dtype = torch.float16 if args.dtype == "f16" else torch.bfloat16
    B, K, Wm = args.batch, args.steps, args.warmup
    H, W = args.height, args.width
    dev = torch.device("cuda", local_rank)
    cfg = ZoeConfig()
    def zoe_weights(variant):
        w_ = random_zoedepth_weights(cfg, seed=args.weights_seed)
        if WEIGHT_VARIANTS[variant] is not None:
            WEIGHT_VARIANTS[variant](w_)
        return w_

    wz = zoe_weights(args.weights)
    wp = random_cyclepose_weights(seed=0)
    strong = args.scaling == "strong"
    if strong:
        from bodyslam_amd.pipeline import shard_bounds
        Nseq = args.frames
        bounds = [shard_bounds(Nseq, world, r) for r in range(world)]
        s0, e0 = bounds[rank]
        # batch: the largest block cut into equal batches of at most --batch frames (125 -> 63 + 62; the last one runs padded)
        nmax = max(e - s for s, e in bounds)
        B = -(-nmax // (-(-nmax // B)))
        foff = max(s0 - 1, 0)
        if args.full:
            frames = torch.from_numpy(make_sequence(Nseq, H, W, seed=0)[foff:e0]).to(dev)    # the rank's block + halo, resident in HBM
        else:
            frames = device_sequence(Nseq, H, W, 0, dev)[foff:e0].clone()
        n_frames = Nseq
    else:
        n_frames = (K + Wm) * B + 1
        if world == 1:
            # (rank 0 at N = 1 with the CPU baseline: the sequence is made on the host first, the oracle reads it, THEN it goes to HBM -- below)
            frames = None
        else:
            # ONE sequence of world x (K + Wm) x B frames (+ the frame before it): step k hands rank r the block of B frames that
            # follows rank r - 1's (its one-frame halo is that block's last frame), so the gathered relatives of a step chain into
            # world x B consecutive poses of the same sequence -- config 4's semantics, weak-scaled.  A rank makes only its own frames.
            from bodyslam_amd.synthetic import make_sequence_at
            total, idx = weak_frame_indices(K + Wm, B, world, rank)
            frames = torch.from_numpy(make_sequence_at(idx, total, H, W, seed=0)).to(dev)
    counts = [B] * world

    def check_samples(K_, Wm_):
        """the (timed step, frame in its batch) pairs whose depth maps are copied out of the timed plan and compared with the oracle:
        N_CHECK_FRAMES of them, spread over the timed steps and over the batch"""
        n = N_CHECK_FRAMES
        if strong:
            return [(K_ - 1, (j * 37) % B) for j in range(n)]
        return sorted({(Wm_ + (j * K_) // n, (j * (B // n) + 3 * j) % B) for j in range(n)})

    # ---- CPU baseline + the oracle's depth maps of the check frames: BEFORE this process touches the GPU (rank 0 at N = 1: the contract)
    cpu, oracle_d, ncores = None, {}, None
    do_cpu = rank == 0 and world == 1 and not args.no_cpu_baseline and not strong
    if do_cpu:
        from oracle import cyclepose_ref as CP
        from oracle import geom3d_ref as G
        from oracle import zoedepth_ref as Z
        # torch CPU ops stop scaling (and then collapse) far below a 256-thread host: use at most 32 threads
        ncores = min(os.cpu_count() or 1, 32)
        torch.set_num_threads(ncores)
        frames_host = torch.from_numpy(make_sequence(n_frames, H, W, seed=0))
        tcpu = 0.0
        for (k_, j_) in check_samples(K, Wm):
            i0 = k_ * B + 1 + j_                                  # index into the sequence: step k's chunk is frames[k*B : (k+1)*B + 1], halo first
            f2 = frames_host[i0 - 1: i0 + 1]
            tc = time.perf_counter()
            with torch.no_grad():
                d_ref = Z.infer_depth(wz, Z.ZOED_NK, f2[1:2], flip_aug=True)
                T = CP.forward_pose(wp, CP.center_crop_pair(f2, torch.tensor([[0, 1]])))
            g_ref = G.pose_chain(T.numpy())
            G.backproject(Z.to_uint16(d_ref)[0], pose=g_ref[1])
            tcpu += time.perf_counter() - tc
            oracle_d[(k_, j_)] = d_ref[0]
        cpu = dict(value=round(len(oracle_d) / tcpu, 4), unit="frames/s", cores=ncores, kind="port",
                   sample=f"{len(oracle_d)} frames {W}x{H} of the timed sequence, each: ZoeD_NK x2 (flip-aug) + 1 CyclePose pair + chain + back-projection, "
                          f"torch fp32 oracle, {tcpu:.1f} s in all, taken before the process's first GPU call")
    # ---- from here on the GPU
    torch.cuda.set_device(local_rank)
    if use_dist:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29511")
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", local_rank))
    if do_cpu:
        frames = frames_host.to(dev)
        del frames_host
    elif frames is None:
        frames = torch.from_numpy(make_sequence(n_frames, H, W, seed=0)).to(dev) if args.full else device_sequence(n_frames, H, W, 0, dev)
    pairs = torch.tensor([[i, i + 1] for i in range(B)], dtype=torch.int32, device=dev)

    def barrier():
        if use_dist:
            dist.barrier()
        torch.cuda.synchronize()

    def measure(precision, wz=wz, K=K, Wm=Wm, host_io=False, pipe=None, samples=(), keep_last=False):
        """W warm-up + K timed steps of the whole loop in one precision mode -> (pipeline, plan, fps, elapsed, rooflines, table).
        host_io: the PCIe-inclusive variant -- every step's frames come from pinned host memory and its depth maps (uint16), point counts and
        relative poses go back to pinned host buffers, all on the compute stream (nothing overlapped: the conservative figure).
        keep_last: the result's "last" holds the last step's outputs (references only: nothing is copied inside the timed steps)."""
        if pipe is None:
            pipe = BodySlamPipeline(wz, wp, cfg, dtype=dtype, device=local_rank, batch=B, precision=precision)
        pipe.calibrate(H, W)        # the correction modes: measured once by rank 0 on the device and shared (every rank runs the same arithmetic)
        zplan = pipe.zoe.plan_for(B, H, W, True)
        pplan = None if strong else pipe.pose.plan_for(B + 1, B, H, W)
        events = []
        snaps = {}          # (step, frame in batch) -> the timed plan's depth map of that frame (samples: compared with the oracle afterwards)

        state = {"g_last": None}
        if host_io:
            h_frames = frames.cpu().pin_memory()
            h_depth = torch.empty(B, H, W, dtype=torch.int16).pin_memory()
            h_cnt = torch.empty(B, dtype=torch.int32).pin_memory()
            h_T = torch.empty(B, 16, dtype=torch.float32).pin_memory()

        def step(k, timed_kernels):
            zplan.plan.events = events if timed_kernels else None
            if strong:      # the whole sequence: this rank's block through run_sequence (all-gather + chain + back-projection inside)
                res = pipe.run_sequence(frames, rank, world, frame_offset=foff, n_frames=Nseq)
                if keep_last:
                    state["last"] = dict(depth_u16=res.depth_u16, t_rel=res.t_rel, g_abs=res.g_abs, counts=res.point_counts)
                return res.point_counts
            chunk = frames[k * B: (k + 1) * B + 1] if world == 1 else frames[weak_chunk(k, B)]     # halo frame + B frames
            if host_io:
                pplan.frames.copy_(h_frames[k * B: (k + 1) * B + 1], non_blocking=True)        # H2D: B + 1 frames, once
                chunk = pplan.frames
            zplan.frames.copy_(chunk[1:])
            zplan.plan.run()
            for (k_, j_) in samples:
                if k_ == k:
                    snaps[(k_, j_)] = zplan.depth_m[j_].clone()          # (1.2 MB device-to-device on the compute stream)
            if not host_io:
                pplan.frames.copy_(chunk)
            pplan.pairs.copy_(pairs)
            pplan.plan.run()
            t_all = gather_relative_poses(pplan.T, counts) if use_dist else pplan.T
            # the chain continues from the previous step's last pose (device-resident g0); at N > 1 every rank chains the
            # gathered block of world x B relatives and keeps its own B poses
            g_abs = geom3d.pose_chain(t_all, g0=state["g_last"], device=local_rank)
            state["g_last"] = g_abs[-1]
            xyz, idx, cnt = geom3d.backproject(zplan.depth_u16, pipe.K, pipe.depth_scale, pipe.depth_trunc,
                                               poses=g_abs[rank * B + 1: (rank + 1) * B + 1])
            if host_io:
                h_depth.copy_(zplan.depth_u16, non_blocking=True)
                h_cnt.copy_(cnt, non_blocking=True)
                h_T.copy_(pplan.T.view(B, 16), non_blocking=True)
            if keep_last:       # (the plan's own buffers hold the last step's maps and relatives until the plan runs again)
                state["last"] = dict(depth_m=zplan.depth_m, depth_u16=zplan.depth_u16, t_rel=pplan.T, g_abs=g_abs, counts=cnt, xyz=xyz, idx=idx)
            return cnt

        for k in range(Wm):
            step(k, False)
        barrier()
        sampler = None
        if rank == 0 and args.full:
            pr = torch.cuda.get_device_properties(local_rank)
            pci = ("%04x:%02x:%02x.0" % (getattr(pr, "pci_domain_id", 0), pr.pci_bus_id, pr.pci_device_id)) if hasattr(pr, "pci_bus_id") else None
            sampler = PowerSampler(pci).start()
        t0 = time.perf_counter()
        for k in range(Wm, Wm + K):
            step(k, not args.no_kernel_timing)
        barrier()
        elapsed = time.perf_counter() - t0
        power = sampler.result() if sampler is not None else None
        zplan.plan.events = None
        if use_dist:
            te = torch.tensor([elapsed], dtype=torch.float64, device=dev)
            dist.all_reduce(te, op=dist.ReduceOp.MAX)
            elapsed = te.item()
        fps = (K * Nseq if strong else world * K * B) / elapsed
        d_timed = {kj: v.cpu() for kj, v in snaps.items()}

        # ---- per-kernel roofline from the HIP events of the timed steps (rank 0's view).  "achieved" counts ALGORITHMIC FLOPs
        # (2*M*N*K of the convolution / GEMM being computed); "executed" counts the MFMA work actually issued, which in
        # accurate mode is 2x (backbone) or 3x (neck, heads) larger because every product is a sum of split-precision passes.
        roof, roof_conv, kern_table = None, None, {}
        if events:
            import re
            agg = {}
            gemm_events = [(ci, e0, e1) for (ci, e0, e1) in events if ci in zplan.plan.gemm_info]
            for (ci, e0, e1) in gemm_events:
                gi = zplan.plan.gemm_info[ci]
                key = ("conv" if gi["conv"] else "gemm", gi["tile"])
                a = agg.setdefault(key, dict(ms=0.0, flops=0.0, alg=0.0, n=0, bytes=0.0))
                a["ms"] += e0.elapsed_time(e1)
                a["flops"] += gi["flops"]
                a["alg"] += gi["alg_flops"]
                a["bytes"] += gi["bytes"]
                a["n"] += 1
            for (kind, tile), a in agg.items():
                kern_table[f"igemm_{kind}_{TILE_NAMES[tile]}"] = dict(
                    launches=a["n"], avg_us=1e3 * a["ms"] / a["n"], tflops=a["alg"] / (a["ms"] * 1e-3) / 1e12,
                    executed_tflops=a["flops"] / (a["ms"] * 1e-3) / 1e12,
                    gflop_per_launch=a["alg"] / a["n"] / 1e9, share_of_step=a["ms"] / (elapsed * 1e3))
            # the same launches by call site (layer index stripped): which GEMM of the network is how far from the roofline
            by = {}
            for (ci, e0, e1) in events:
                gi = zplan.plan.gemm_info.get(ci) or zplan.plan.stack_info[ci]
                nm = re.sub(r"^(l|rt|ro|ra|nc|fu|pj|at)\d+", r"\1*", gi["name"])
                a = by.setdefault(nm, dict(ms=0.0, alg=0.0, ex=0.0, n=0))
                a["ms"] += e0.elapsed_time(e1); a["alg"] += gi["alg_flops"]; a["ex"] += gi["flops"]; a["n"] += 1
            for nm, a in sorted(by.items(), key=lambda kv: -kv[1]["ms"])[:14]:
                kern_table["site:" + nm] = dict(launches=a["n"], avg_us=round(1e3 * a["ms"] / a["n"], 1), tflops=round(a["alg"] / a["ms"] / 1e9, 1),
                                                executed_tflops=round(a["ex"] / a["ms"] / 1e9, 1), share_of_step=round(a["ms"] / (elapsed * 1e3), 4))
            dom = max(agg.items(), key=lambda kv: kv[1]["ms"])
            (kind, tile), a = dom
            ach = a["alg"] / (a["ms"] * 1e-3) / 1e12
            exe = a["flops"] / (a["ms"] * 1e-3) / 1e12
            # HBM bytes per launch of that kernel from the committed PMC collection (separate --pmc passes, FETCH_SIZE doubled as
            # the microarch guide prescribes for gfx950); only valid for the batch / mode it was collected at
            # HBM bytes per launch of that kernel: PMC counters of the child runs above (2 * FETCH_SIZE + WRITE_SIZE: gfx950's
            # FETCH_SIZE counts 64 of every 128 streamed bytes, /opt/skills/guides/MI355X_MICROARCH.md "HBM"; values are KB)
            traffic, traffic_source = None, None
            if pmc and precision == args.precision:
                mode = {"gemm": "ELi0E", "conv": "ELi1E"}[kind]
                dims = TILE_NAMES[tile].split("s")[0].split("x")
                cands = [v for name, v in pmc.items()
                         if ("igemm_kernel" in name and f"Li{dims[0]}ELi{dims[1]}E" in name and f"Li{dims[2]}E" in name and mode in name
                             and ("DF16_" in name) == (args.dtype == "f16"))]
                if cands:       # the F8 / plain instantiation with the most launches is the one the events timed
                    n_l, f_kb, w_kb = max(cands, key=lambda v: v[0])
                    traffic = round((2.0 * f_kb + w_kb) * 1024.0)
                    traffic_source = ("rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE, two child runs of this command (1 step) before the timed "
                                      "run; (2*FETCH_SIZE + WRITE_SIZE) KB per launch, mean over the kernel's launches of at least a tenth of its largest "
                                      "grid (the plan's; the calibration's four-frame launches of the same instantiation are left out)")
            roof = dict(bound="mfma", kernel=f"igemm_kernel<{args.dtype},{TILE_NAMES[tile]},{kind}>", achieved=round(ach, 1),
                        peak=MFMA_PEAK_TFLOPS, unit="TFLOP/s", frac=round(ach / MFMA_PEAK_TFLOPS, 4), traffic=traffic, traffic_source=traffic_source,
                        executed=round(exe, 1), executed_frac=round(exe / MFMA_PEAK_TFLOPS, 4),
                        avg_launch_us=round(1e3 * a["ms"] / a["n"], 2), gflop_per_launch=round(a["alg"] / a["n"] / 1e9, 3),
                        algorithmic_bytes_per_launch=round(a["bytes"] / a["n"]))
            if power and power.get("sclk_mhz_median"):
                # `peak` is the guide's figure at the 2.4 GHz boost clock; the plan runs at the board's power limit and a lower clock
                roof["sclk_mhz_median"] = power["sclk_mhz_median"]
                roof["frac_of_peak_at_that_clock"] = round(ach / (MFMA_PEAK_TFLOPS * power["sclk_mhz_median"] / 2400.0), 4)
            # ---- the conv stack of SURVEY section 8(d) -- neck + relative head + metric head + patch embedding, 233.6 GFLOP per forward in the
            # reference's formulation -- as EVERY launch that carries a piece of it: all bs_gemm launches outside the 24 BEiT layers and the
            # readout Linears, plus the fused up-convolution and the attractor MLP kernels (Plan.stack_info).  `achieved` prices the
            # reference's 233.6 GFLOP x forwards against their summed time (VERDICT r5 #1 i); `as_launched` counts the products as this plan
            # evaluates them (linear maps moved to the low resolution, composed, tap products: fewer FLOPs for the same result);
            # `conv_mode_only` is rounds 1-5's figure (the 3x3 launches alone).
            in_stack = lambda nm_: not re.match(r"^(l\d+\.|ro\d)", nm_)
            st = dict(ms=0.0, alg=0.0, ex=0.0, n=0)
            for (ci, e0, e1) in events:
                gi = zplan.plan.gemm_info.get(ci) or zplan.plan.stack_info[ci]
                if in_stack(gi["name"]):
                    st["ms"] += e0.elapsed_time(e1); st["alg"] += gi["alg_flops"]; st["ex"] += gi["flops"]; st["n"] += 1
            cms = sum(a["ms"] for (kd, _), a in agg.items() if kd == "conv")
            cfl = sum(a["alg"] for (kd, _), a in agg.items() if kd == "conv")
            cex = sum(a["flops"] for (kd, _), a in agg.items() if kd == "conv")
            if st["ms"] > 0:
                g_ = zplan.geom
                first_ci = min(zplan.plan.gemm_info)                       # the plan's first GEMM: once per plan run (a strong-scaling step runs the plan once per batch)
                forwards = sum(1 for (ci, _, _) in events if ci == first_ci) * g_["NB"]
                ref_gflop = CONV_STACK_GFLOP_PER_FORWARD * (g_["nh"] * g_["nw"]) / (384.0 * 512.0)
                tf = lambda fl, ms: fl / (ms * 1e-3) / 1e12
                ach_s = tf(ref_gflop * 1e9 * forwards, st["ms"])
                roof_conv = dict(bound="mfma", what="ZoeDepth conv stack, WHOLE (SURVEY 8(d): neck + relative head + metric head + patch embed): every launch "
                                                    "that carries a piece of it, incl. bs_upconv_fused and bs_mlp2_add",
                                 achieved=round(ach_s, 1), peak=MFMA_PEAK_TFLOPS, unit="TFLOP/s", frac=round(ach_s / MFMA_PEAK_TFLOPS, 4),
                                 gflop_per_forward_reference=round(ref_gflop, 1), forwards=forwards, launches=st["n"], ms_per_step=round(st["ms"] / K, 3),
                                 as_launched=dict(gflop_per_forward=round(st["alg"] / forwards / 1e9, 1), achieved=round(tf(st["alg"], st["ms"]), 1),
                                                  frac=round(tf(st["alg"], st["ms"]) / MFMA_PEAK_TFLOPS, 4)),
                                 executed=round(tf(st["ex"], st["ms"]), 1), executed_frac=round(tf(st["ex"], st["ms"]) / MFMA_PEAK_TFLOPS, 4),
                                 conv_mode_only=(dict(achieved=round(tf(cfl, cms), 1), frac=round(tf(cfl, cms) / MFMA_PEAK_TFLOPS, 4),
                                                      executed_frac=round(tf(cex, cms) / MFMA_PEAK_TFLOPS, 4), ms_per_step=round(cms / K, 3)) if cms > 0 else None))
        return dict(pipe=pipe, zplan=zplan, fps=fps, elapsed=elapsed, roof=roof, roof_conv=roof_conv, kern=kern_table, d_timed=d_timed, power=power,
                    last=state.get("last"))

    samples = sorted(oracle_d)
    main_run = measure(args.precision, samples=samples, keep_last=args.dump_outputs is not None)
    if args.dump_outputs is not None and rank == 0:      # (before any other leg runs a plan again)
        dump_outputs(args.dump_outputs, main_run.pop("last"), H, W)
    pipe, zplan, fps, elapsed = main_run["pipe"], main_run["zplan"], main_run["fps"], main_run["elapsed"]
    roof, roof_conv, kern_table = main_run["roof"], main_run["roof_conv"], main_run["kern"]
    other = None
    if not args.single_mode:
        other_name = "fast" if args.precision == "accurate" else "accurate"
        other = measure(other_name, samples=samples)
        other.pop("pipe"), other.pop("zplan")             # (its plan's buffers go back to the allocator before the next leg)
        torch.cuda.empty_cache()

    extra_legs = rank == 0 and world == 1 and not strong and args.precision == "accurate" and not args.single_mode
    # ---- PCIe-inclusive rate (never `value`): the same loop with every step's frames uploaded from pinned host memory and its results
    # (uint16 depth maps, point counts, relative poses) copied back, on the compute stream
    pcie = None
    if extra_legs and not args.no_pcie_leg:
        r_ = measure(args.precision, K=min(K, 4), Wm=1, host_io=True, pipe=pipe)        # (the main run's pipeline and plans)
        pcie = {"value": round(r_["fps"], 2), "unit": "frames/s", "ms_per_step": round(1e3 * r_["elapsed"] / min(K, 4), 3),
                "what": f"per step: {B + 1} frames H2D from pinned host memory ({(B + 1) * H * W * 3 / 1e6:.0f} MB), {B} uint16 depth maps + counts + "
                        f"poses D2H ({B * H * W * 2 / 1e6:.0f} MB), copies on the compute stream (not overlapped)"}
        del r_
    # ---- the accurate mode on weights that look trained: 6 outlier channels x 50 behind every LayerNorm.  The calibration
    # has to switch corrections back on there; this is what the tolerance then costs.  Its depth error is taken against the fp32 oracle
    # on the same weights, like the headline's (below, with the CPU baseline).
    outl = None
    if extra_legs and not args.no_outlier_leg and args.weights == "gaussian":
        wz_o = zoe_weights("outlier")
        r_ = measure("accurate", wz=wz_o, K=min(K, 4), Wm=1, samples=sorted({(1, 5 % B), (1, B // 2), (min(K, 4), B // 3), (min(K, 4), B - 1)}))
        zo = r_["pipe"].zoe
        outl = {"weights": "random-init + 6 channels x 50 behind every LayerNorm (bodyslam_amd.synthetic.outlier_channels)",
                "value": round(r_["fps"], 2), "unit": "frames/s", "ms_per_step": round(1e3 * r_["elapsed"] / min(K, 4), 3),
                "class_modes": dict(zo.class_modes), "attn_mode": zo.attn_mode, "neck_mode": zo.neck_mode,
                "l1_abs_vs_reference_m": (zo.calibration or {}).get("l1_abs_vs_reference_m"), "warning": (zo.calibration or {}).get("warning"),
                "l1_backbone_choice_vs_reference_m": (zo.calibration or {}).get("l1_backbone_choice_vs_reference_m"),
                "calibration_holdout": (zo.calibration or {}).get("holdout"),
                "neck_sites": {k_: v_ for k_, v_ in ((zo.calibration or {}).get("neck_sites") or {}).items() if k_ in
                               ("tol_abs_m", "plain_tol_abs_m", "weight_only", "plain", "flops_share_weight_only", "flops_share_plain", "l1_weight_only_m", "l1_plain_m")},
                "executed_gflop_per_input": (zo.calibration or {}).get("executed_gflop_per_input"),
                "roofline_frac": (r_["roof"] or {}).get("frac"), "conv_stack_frac": (r_["roof_conv"] or {}).get("frac")}
        outl_d = r_["d_timed"]
        zo_cal = dict(zo.calibration or {})
        r_.pop("pipe"), r_.pop("zplan")
        del r_, zo
        torch.cuda.empty_cache()

    # ---- the reference's whole per-frame loop around the hot path (BodySlamPipeline.run_slam_loop: + RGB-D odometry and UKF fusion, pose
    # graph every 500 frames, TSDF map at the reference's parameters), reported beside the metric, never as `value`: rank 0 at N = 1
    slam = None
    if rank == 0 and world == 1 and not strong and not args.no_slam_loop and args.precision == "accurate":
        from bodyslam_amd.tsdf import TSDF
        # whole batches only (a ragged last batch runs through the full-size plan and would be timed as B frames: --steps 2 gave 193 frames =
        # 3 batches + 1 frame and read 250 frames/s where 256 frames read 318)
        nloop = max(min(int(frames.shape[0]), 256) // B, 1) * B          # 256 frames (the configs' sequence length) in whole batches
        nloop = min(nloop, int(frames.shape[0]))
        pipe.run_slam_loop(frames[:min(B + 2, nloop)], vo=True, tsdf=TSDF(device=local_rank))       # plans, odometry buffers (not timed)
        torch.cuda.empty_cache()
        # three passes, each into a fresh map (reserved outside the timed region); `value` is the MEDIAN, every pass is listed: the
        # figure moved by 20 % between boxes / process states in round 3, a single pass does not say which
        dts, units = [], 0
        for _ in range(3):
            tsdf = TSDF(device=local_rank)
            tsdf.reserve(4096)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            pipe.run_slam_loop(frames[:nloop], vo=True, tsdf=tsdf, posegraph_every=500)
            torch.cuda.synchronize()
            dts.append(time.perf_counter() - t0)
            units = int(pipe.last_tsdf.n_units)
            del tsdf
            pipe.last_tsdf = None
            torch.cuda.empty_cache()
        dt = sorted(dts)[1]
        slam = {"what": "SLAM._sequential_loop order (3DM/slam.py:131-205): MDEM + MPEM + RGB-D odometry / UKF fusion + chain + pose graph "
                        "every 500 + TSDF map (1 mm voxels, 0.1 m truncation, 32^3 units) + back-projection, one GPU",
                "value": round(nloop / dt, 1), "unit": "frames/s", "frames": nloop, "batch": B, "ms_per_frame": round(1e3 * dt / nloop, 3),
                "passes_frames_per_s": [round(nloop / d, 1) for d in dts], "statistic": "median of 3 passes", "best": round(nloop / min(dts), 1),
                "map_units": units}

    # ---- accuracy of the TIMED plans: the check frames (copied out of the timed steps) against the oracle's maps made before the GPU was touched
    l1 = l1_frames = None

    def frame_stats(dt_):
        per = [float((dt_[kj] - oracle_d[kj]).abs().mean()) for kj in sorted(dt_) if kj in oracle_d]
        if not per:
            return None
        return {"mean": float(np.mean(per)), "max": float(np.max(per)), "min": float(np.min(per)), "n": len(per),
                "per_pixel_max": float(max((dt_[kj] - oracle_d[kj]).abs().max() for kj in dt_ if kj in oracle_d)),
                "frames": [f"step {k_} frame {j_}" for (k_, j_) in sorted(dt_) if (k_, j_) in oracle_d]}

    if do_cpu:
        l1_frames = frame_stats(main_run["d_timed"])
        l1 = l1_frames["mean"] if l1_frames else None
        if other:
            st_o = frame_stats(other["d_timed"])
            other["l1"] = st_o["mean"] if st_o else None
            other["l1_max"] = st_o["max"] if st_o else None
        if outl is not None and outl_d:        # the outlier-weights leg against the oracle ON THOSE WEIGHTS: four frames of its timed steps
            from oracle import zoedepth_ref as Z
            per = []
            for (k_, j_) in sorted(outl_d):
                i_o = k_ * B + 1 + j_
                with torch.no_grad():
                    d_ref_o = Z.infer_depth(wz_o, Z.ZOED_NK, frames[i_o: i_o + 1].cpu(), flip_aug=True)
                per.append(float((outl_d[(k_, j_)] - d_ref_o[0]).abs().mean()))
            outl["depth_l1_vs_oracle_m"] = float(np.max(per))
            outl["depth_l1_frames"] = {"max": float(np.max(per)), "mean": float(np.mean(per)), "min": float(np.min(per)), "n": len(per)}
            outl["tolerance_met"] = bool(np.max(per) <= 1e-4)
            outl["margin_note"] = (zo_cal or {}).get("margin_note")

    # ---- the surface the reference calls: one frame per call.  infer_depth_map = one B = 1 forward (flip-aug) + the uint16 map
    # back on the host; infer_relative_pose_between = one pair.  Frames resident on the device (the interface's own H2D of 0.9 MB is not in it).
    latency = None
    if rank == 0 and world == 1 and not strong and not args.single_mode and not args.no_latency_leg:
        z_, p_ = pipe.zoe, pipe.pose
        f1 = frames[1:2].contiguous()
        lat = {}
        for name, graph in (("infer_depth_map_eager_ms", False), ("infer_depth_map_ms", True)):
            for _ in range(3):
                z_.infer(f1, graph=graph)[1][0].cpu()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(20):
                z_.infer(f1, graph=graph)[1][0].cpu()           # (the call's own synchronisation: the map comes back to the host)
            lat[name] = round(1e3 * (time.perf_counter() - t0) / 20, 3)
        pr1 = torch.tensor([[0, 1]], dtype=torch.int32, device=dev)
        f2_ = frames[0:2].contiguous()
        for _ in range(3):
            p_.infer_pairs(f2_, pr1).cpu()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(20):
            p_.infer_pairs(f2_, pr1).cpu()
        lat["infer_relative_pose_between_ms"] = round(1e3 * (time.perf_counter() - t0) / 20, 3)
        lat["what"] = ("wall time per call, mean of 20: B = 1 ZoeD_NK forward x2 (flip-aug) replayed as one HIP graph + uint16 map D2H; eager = ~500 ctypes "
                       "launches per call; one CyclePose pair + 4x4 D2H; frames resident on the device")
        latency = lat

    if rank == 0:
        out = {
            "metric": f"frames/sec depth+pose+back-proj, {W}x{H} seq", "value": round(fps, 2), "unit": "frames/s",
            "n_gpus": world, "steps": K, "warmup": Wm, "ms_per_step": round(1e3 * elapsed / K, 3), "higher_is_better": True,
            "scaling": args.scaling, "vs_baseline": None, "dtype": args.dtype, "data": "synthetic frames, random-init weights",
            "config": ({"workload": f"full MDEM(ZoeD_NK, flip-aug)+MPEM(CyclePose)+3DM loop, ONE {Nseq}-frame synthetic {W}x{H} sequence cut "
                                    f"into {world} contiguous block(s), batch {B} frames (ragged last batch padded)",
                        "sequence_frames": Nseq, "frames_per_step": Nseq, "batch": B, "net_input": list(zplan.geom[k] for k in ("nh", "nw")),
                        "sharding": {"blocks": [e - s for s, e in bounds], "halo_frames": 1,
                                     "exchange": "one RCCL all-gather of the [N_r,16] relative poses per sequence" if world > 1 else "none (single GPU)"}}
                       if strong else
                       {"workload": f"full MDEM(ZoeD_NK, flip-aug)+MPEM(CyclePose)+3DM loop, {K * B} synthetic {W}x{H} frames per GPU, "
                                    f"batch {B} frames/step", "frames_per_step_per_gpu": B, "net_input": list(zplan.geom[k] for k in ("nh", "nw")),
                        "sharding": "ONE sequence: per step, rank r owns the B frames after rank r-1's (1-frame halo); one RCCL all-gather of the relative poses per step" if world > 1 else "single GPU"}),
            "roofline": roof, "cpu_baseline": cpu,
            # per-instantiation / per-site table of the timed GEMM launches and the calibration's full report: the bulky parts come FIRST, the
            # figures a reviewer needs are the LAST ~1500 characters of the line (the driver keeps the tail)
            "kernels": kern_table,
            # (the static bias corrections travel in the report for the other ranks: here only how many values each site carries)
            "calibration": ({k_: (v_ if k_ not in ("site_bias_corr", "backbone_bias_corr") else {"products": len(v_), "values": sum(len(c_) for c_ in v_.values())})
                             for k_, v_ in (pipe.zoe.calibration or {}).items()}
                            if pipe.zoe.acc else None),
            "hbm_allocated_gb": round(torch.cuda.max_memory_allocated() / 2 ** 30, 1),
            "power": main_run.get("power"),
            "full": args.full,
        }
        if slam:
            out["slam_loop"] = slam
        if other:
            out["other_mode"] = {"precision": other_name, "value": round(other["fps"], 2), "unit": "frames/s",
                                 "ms_per_step": round(1e3 * other["elapsed"] / K, 3), "depth_l1_vs_oracle_m": other.get("l1"),
                                 "depth_l1_max_over_frames_m": other.get("l1_max"),
                                 "roofline_frac": (other["roof"] or {}).get("frac"), "conv_stack_frac": (other["roof_conv"] or {}).get("frac")}
        if outl is not None:
            out["outlier_weights"] = outl
        if pcie is not None:
            out["pcie_inclusive"] = pcie
        # ---- the tail: precision, accuracy of the timed plan, conv-stack roofline, the modes the calibration chose (+ its absolute check)
        zc = pipe.zoe.calibration or {}
        out["precision"] = args.precision
        out["weights"] = args.weights
        out["weights_seed"] = args.weights_seed
        ns_ = zc.get("neck_sites") or {}
        nm_ = pipe.zoe.neck_mode if pipe.zoe.acc else ""
        # (the full neck mode string is in `calibration` above; the tail carries its size)
        out["accurate_modes"] = ({"class_modes": pipe.zoe.class_modes, "attn_mode": pipe.zoe.attn_mode,
                                  "neck": (nm_ if len(nm_) < 40 else {"weight_only_sites": len(nm_.split(";")[0].split(",")),
                                                                      "one_pass_sites": (len(nm_.split(";plain:")[1].split(",")) if ";plain:" in nm_ else 0),
                                                                      "flops_share_weight_only": ns_.get("flops_share_weight_only"),
                                                                      "flops_share_one_pass": ns_.get("flops_share_plain")}),
                                  "l1_abs_vs_reference_m": zc.get("l1_abs_vs_reference_m"), "warning": zc.get("warning")} if pipe.zoe.acc else None)
        out["slam_loop_frames_per_s"] = slam["value"] if slam else None
        out["latency_b1_ms"] = latency
        out["calibrate_s"] = zc.get("calibrate_s")
        out["calibration_holdout"] = ({k_: zc["holdout"][k_] for k_ in ("frames", "tol_m", "l1_max_m", "l1_mean_m", "withdrawn")} if "holdout" in zc else None)
        out["roofline_conv_stack"] = roof_conv
        # accuracy of the TIMED plan: N_CHECK_FRAMES frames spread over the timed steps, each against the fp32 CPU oracle; `value` is a
        # tolerance-meeting figure only while depth_l1_frames.max <= 1e-4 m (the north star's tolerance)
        out["depth_l1_vs_oracle_m"] = l1
        out["depth_l1_frames"] = ({k_: l1_frames[k_] for k_ in ("mean", "max", "min", "n", "per_pixel_max")} if l1_frames else None)
        out["depth_l1_frame"] = (", ".join(l1_frames["frames"]) + " of the timed plan's output" if l1_frames else None)
        out["tolerance_met"] = (bool(l1_frames["max"] <= 1e-4) if (l1_frames and args.precision != "fast") else None)
        print(json.dumps(out))
    if use_dist:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
