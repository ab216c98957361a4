"""Record tests/golden/calibration_traces.json from a checkout of the commit BEFORE calibrate() was split into calibration.py's stages:
    git worktree add <dir> <that commit>;  python tools/make_calibration_traces.py <dir>
Runs every scenario of tests/_calibration_fake.py through <dir>'s ZoeDepthEngine.calibrate on the CPU (the fake stands in for the device)
and writes, per scenario, the ordered measurement calls, the warnings and the final report.  A line trace checks first that the
scenarios reach every statement of that calibrate(); the lines they do not reach are printed.  The file is generated from that commit,
never from the code under test (tests/test_calibration_cpu.py replays it); the script is kept so the provenance can be redone."""
import importlib.util
import inspect
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
parent = os.path.abspath(sys.argv[1])
sys.path.insert(0, parent)
import bodyslam_amd.zoedepth as ZD  # noqa: E402

assert os.path.dirname(os.path.dirname(os.path.abspath(ZD.__file__))) == parent, ZD.__file__
spec = importlib.util.spec_from_file_location("_calibration_fake", os.path.join(ROOT, "tests", "_calibration_fake.py"))
fake = importlib.util.module_from_spec(spec)
spec.loader.exec_module(fake)

src, first = inspect.getsourcelines(ZD.ZoeDepthEngine.calibrate)
fname, last, reached = ZD.ZoeDepthEngine.calibrate.__code__.co_filename, first + len(src) - 1, set()


def line_trace(frame, event, arg):
    if event == "line":
        reached.add(frame.f_lineno)
    return line_trace


def call_trace(frame, event, arg):          # calibrate() and the closures defined inside it
    return line_trace if frame.f_code.co_filename == fname and first <= frame.f_code.co_firstlineno <= last else None


out = {"parent_commit": subprocess.check_output(["git", "-C", parent, "rev-parse", "HEAD"], text=True).strip(), "neck_modes": [], "scenarios": {}}
for name in fake.SCENARIOS:
    sys.settrace(call_trace)
    try:
        got = fake.run_scenario(ZD, name)
    finally:
        sys.settrace(None)
    for call in got["calls"]:                # each distinct neck-mode string is stored once
        if call[1] not in out["neck_modes"]:
            out["neck_modes"].append(call[1])
        call[1] = out["neck_modes"].index(call[1])
    out["scenarios"][name] = got
    rep = got["report"]
    print(f"{name}: {len(got['calls'])} measurements, {rep['class_modes']} attn {rep['attn_mode']} neck {rep['neck_mode'][:60]} "
          f"withdrawn {rep.get('holdout', {}).get('withdrawn')} {[k for k in rep if 'note' in k or k == 'warning']}")
missed = [first + i for i, l in enumerate(src) if first + i not in reached and l.strip() and not l.strip().startswith(("#", '"""'))]
print("lines of calibrate() no scenario reached:")
for n in missed:
    print(f"  {n}: {src[n - first].rstrip()[:150]}")
path = os.path.join(ROOT, "tests", "golden", "calibration_traces.json")
with open(path, "w") as f:
    json.dump(out, f, separators=(",", ":"))
print(f"wrote {path}: {os.path.getsize(path)} bytes")
