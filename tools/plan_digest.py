"""A canonical, address-free text form of a ZoeDepth plan: "the plan is unchanged" as a diff of two files.

    python tools/plan_digest.py --row full_fixed                # digests of one row of the matrix on stdout
    python tools/plan_digest.py --matrix DIR                    # one file per case of the matrix, every row in a child process of its own

One line per launch: call index, plan name, entry point, every argument -- integers and floats as they are, device pointers as
(buffer ordinal, byte offset).  Buffers are the distinct storages reachable from Plan.keep, the marks and the plan's I/O tensors, numbered
in order of first appearance in the call stream; a buffer's size is printed where it first appears.  A bs_gemm launch prints every
bs_gemm_desc field by name.  Then the marks, gemm_info, stack_info, site_flops, geom and the pool's size.  Two trees that print the same
digest launch the same kernels with the same arguments over the same buffer layout.

Nothing is launched except what building the engine launches (weight ingestion, and the calibration of an "auto" engine).  Only
attributes that every revision of the plan has are read (calls, names, keep, keep_descs, marks, gemm_info, stack_info), so the file can be
copied into an older tree and run there.  A row is one engine; the rows that depend on an environment switch set it in the child.
"""
import argparse
import ctypes as C
import dataclasses
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _num(v):
    return repr(float(v)) if isinstance(v, float) else str(int(v))


class _Locator:
    """device pointer -> "b<ordinal>+<offset>", ordinals in order of first use"""

    def __init__(self, bufs):
        self.bufs, self.ordinal = bufs, {}

    def __call__(self, ptr, what):
        if not ptr:
            return "null"
        i, off = self.bufs.locate(int(ptr), what)
        new = i not in self.ordinal
        n = self.ordinal.setdefault(i, len(self.ordinal))
        return f"b{n}+{off}" + (f"[{self.bufs.size[i]}]" if new else "")


def digest(zp) -> str:
    """the digest of a _ZoePlan"""
    from bodyslam_amd import _lib as L
    from bodyslam_amd import engine_export as X
    P = zp.plan
    ts = []
    X._tensors(P.keep, ts)
    X._tensors([t for ms in P.marks.values() for (_, t, _) in ms], ts)
    X._tensors([zp.frames, zp.depth_m, zp.depth_u16, zp.depth_net, zp.logits, zp.route], ts)
    loc = _Locator(X._Buffers(ts, set()))
    out = []
    gi = 0
    for i, (fn, args) in enumerate(P.calls):
        if isinstance(fn, str):                      # (a stream fork / join of an older tree's second lane)
            out.append(f"{i} {P.names[i]} {fn} {args}")
            continue
        name = fn.__name__
        if name == "bs_gemm":
            d = P.keep_descs[gi]
            gi += 1
            fields = []
            for fname, ty in L.GemmDesc._fields_:
                v = getattr(d, fname)
                fields.append(f"{fname}={loc(v, fname) if ty is C.c_void_p else _num(v)}")
            out.append(f"{i} {P.names[i]} {name} " + " ".join(fields))
            continue
        sig = L._SIGS[name][:-1]
        assert len(sig) == len(args), (name, len(sig), len(args))
        out.append(f"{i} {P.names[i]} {name} " + " ".join(loc(a, name) if ty is C.c_void_p else _num(a) for ty, a in zip(sig, args)))
    for i in sorted(P.marks):
        for (name, t, meta) in P.marks[i]:
            out.append(f"mark {i} {name} {meta!r} {loc(t.data_ptr(), name)}")
    for title, info in (("gemm_info", P.gemm_info), ("stack_info", P.stack_info)):
        for i in sorted(info):
            out.append(f"{title} {i} " + " ".join(f"{k}={info[i][k]!r}" for k in sorted(info[i])))
    for k in sorted(zp.site_flops):
        out.append(f"site_flops {k} {zp.site_flops[k]!r}")
    out.append("geom " + " ".join(f"{k}={zp.geom[k]}" for k in sorted(zp.geom)) + f" grouped={zp.grouped} attn_corr={zp.attn_corr}")
    out.append(f"pool bytes_new={zp.pool.bytes_new} blocks={len(zp.pool.blocks)}")
    return "\n".join(out) + "\n"


# ---- the matrix: row name -> (environment of the child, builder).  A builder yields (case name, engine, (B, H, W, flip)).
FIXED = dict(class_modes={"qkv": "full", "o": "full", "fc1": "full", "fc2": "full"}, attn_mode="corr", neck_mode="full")
VGA = (480, 640)


def _full(cfg_name="ZOED_NK", **kw):
    import torch
    from bodyslam_amd import zoedepth as Z
    from bodyslam_amd.synthetic import random_zoedepth_weights
    cfg = getattr(Z, cfg_name)
    kw.setdefault("dtype", torch.float16)
    return Z.ZoeDepthEngine(random_zoedepth_weights(cfg, seed=0), cfg, **kw)


def _small(seed=4, **kw):
    """the small backbone with the full-size neck and heads (tests/test_zoedepth_gpu.py small_oracle_cfg / product_cfg)"""
    import torch
    from bodyslam_amd import zoedepth as Z
    from oracle import zoedepth_ref as R
    over = {k: kw.pop(k) for k in ("head_names", "add_projection") if k in kw}
    cfg_o = R.ZoeConfig(hidden=128, layers=4, heads=2, intermediate=256, taps=(1, 2, 3, 4), image_size=64, **over)
    names = {f.name for f in dataclasses.fields(Z.ZoeConfig)}
    cfg = Z.ZoeConfig(**{k: v for k, v in dataclasses.asdict(cfg_o).items() if k in names})
    return Z.ZoeDepthEngine(R.synth_weights(cfg_o, seed=seed), cfg, dtype=torch.float16, target_hw=(96, 128), **kw)


def row_full_fast():
    e = _full(precision="fast")
    yield "b1", e, (1, *VGA, True)
    yield "b4_noflip", e, (4, *VGA, False)


def row_full_fixed():
    e = _full(precision="accurate", **FIXED)
    yield "b1", e, (1, *VGA, True)
    yield "b64", e, (64, *VGA, True)
    for m in ("wcls", "wmean"):
        e.set_class_modes({k: m for k in FIXED["class_modes"]}, "w", "single")
        yield "b4_" + m, e, (4, *VGA, True)


def row_full_fixed_b1():
    yield "b1", _full(precision="accurate", **FIXED), (1, *VGA, True)


def row_full_auto():
    e = _full(precision="accurate")
    yield "b4", e, (4, *VGA, True)
    yield "b1_320x320", e, (1, 320, 320, True)          # 384 x 384 network input: image-major rows
    yield "b2_720x1280", e, (2, 720, 1280, True)        # 384 x 672: image-major rows


def row_full_auto_b4():
    yield "b4", _full(precision="accurate"), (4, *VGA, True)


def row_full_reference():
    yield "b1", _full(precision="reference"), (1, *VGA, True)


def row_full_bf16():
    import torch
    yield "b1", _full(precision="accurate", dtype=torch.bfloat16, **FIXED), (1, *VGA, True)


def row_full_single_head():
    yield "b1", _full("ZOED_N", precision="accurate", **FIXED), (1, *VGA, True)


def row_small():
    g = (3, 120, 160, True)
    yield "fixed", _small(precision="accurate", **FIXED), g
    # every neck site one-pass, as tests/test_zoedepth_gpu.py::test_no_launch_reads_memory_the_plan_has_not_written builds it
    e = _small(precision="accurate", class_modes="full", attn_mode="single", neck_mode="full")
    sites = sorted(k for k in e.f8s if not (k[0] == "l" and k[1].isdigit()) and k != "pe.w" and not k.endswith("w_cls") and not k.startswith("mh."))
    e.set_class_modes({}, "wonly:" + ",".join(sites) + ";plain:" + ",".join(k for k in sites if k != "rh.conv2.w"))
    yield "one_pass", e, g
    yield "no_projection", _small(seed=6, precision="accurate", add_projection=False, **FIXED), g
    yield "fast", _small(precision="fast"), g
    # the probe modes of the backbone classes ("a", "single", "w": ingestion-time choices)
    yield "probe_modes", _small(precision="accurate", class_modes={"qkv": "a", "o": "single", "fc1": "full", "fc2": "w"}, attn_mode="single",
                                neck_mode="full"), g


def row_small_single_head():
    for precision in ("accurate", "fast"):
        yield precision, _small(seed=5, precision=precision, head_names=("nyu",)), (2, 120, 160, True)


ROWS = {
    "full_fast": ({}, row_full_fast),
    "full_fixed": ({}, row_full_fixed),
    "full_auto": ({}, row_full_auto),
    "full_auto_wstat": ({"BS_AUTO_WSTAT": "1"}, row_full_auto_b4),
    "full_reference": ({}, row_full_reference),
    "full_bf16": ({}, row_full_bf16),
    "full_single_head": ({}, row_full_single_head),
    "small": ({}, row_small),
    "small_single_head": ({}, row_small_single_head),
    "full_fixed_projector_level0": ({"BS_PROJECTOR_LEVEL": "0"}, row_full_fixed_b1),
    "full_fixed_upconv_fused0": ({"BS_UPCONV_FUSED": "0"}, row_full_fixed_b1),
    "full_fixed_mlp2_1": ({"BS_MLP2": "1"}, row_full_fixed_b1),
    "full_fixed_mlp2_0": ({"BS_MLP2": "0"}, row_full_fixed_b1),
    "full_fixed_neck_bias_corr0": ({"BS_NECK_BIAS_CORR": "0"}, row_full_fixed_b1),
}


def run_row(row: str, out_dir=None):
    import torch
    from bodyslam_amd.zoedepth import _ZoePlan
    env, builder = ROWS[row]
    assert all(os.environ.get(k) == v for k, v in env.items()), f"row {row} wants {env} in the environment (--matrix sets it)"
    for case, eng, (B, H, W, flip) in builder():
        if eng.auto_modes and eng.calibration is None:       # (what plan_for does in front of an engine's first plan)
            eng.calibrate(H, W)
        zp = _ZoePlan(eng, B, H, W, flip)
        head = f"# {row}.{case} B={B} H={H} W={W} flip={flip} class_modes={sorted(eng.class_modes.items())} attn_mode={eng.attn_mode} neck_mode={eng.neck_mode}\n"
        text = head + digest(zp)
        if out_dir:
            os.makedirs(out_dir, exist_ok=True)
            with open(os.path.join(out_dir, f"{row}.{case}.txt"), "w") as f:
                f.write(text)
            print(f"{row}.{case}: {len(zp.plan.calls)} launches", flush=True)
        else:
            sys.stdout.write(text)
        del zp
        torch.cuda.empty_cache()


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--row", choices=sorted(ROWS), help="one row of the matrix, in this process")
    ap.add_argument("--matrix", metavar="DIR", help="every row, one child process after the other; one digest file per case in DIR")
    ap.add_argument("--rows", default="", help="with --matrix: a comma-separated subset of the rows")
    ap.add_argument("--out", metavar="DIR", help="with --row: write the digests into DIR instead of stdout")
    a = ap.parse_args(argv)
    if a.row:
        return run_row(a.row, a.out)
    assert a.matrix, "give --row or --matrix"
    for row in (a.rows.split(",") if a.rows else ROWS):
        env = dict(os.environ, **ROWS[row][0])
        # (one engine at a time: full-size weights are 1.4 GB on the host, and BS_MLP2 is read when the engine is constructed)
        subprocess.run([sys.executable, sys.argv[0], "--row", row, "--out", a.matrix], env=env, check=True, timeout=900)


if __name__ == "__main__":
    main()
