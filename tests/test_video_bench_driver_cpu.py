"""No-GPU checks of tools/video_bench.py, the module under the streamed-video benchmarks: the step driver (one child process per step
under its own `timeout`, the record file, nothing started after a step that failed or ran into its limit), the flags it hands on, the
summaries of the timers on a fake clock, and that each of the 14 tools answers --help without importing torch.  The steps of the stand-in
tool print, exit, sleep or touch a file; nothing here opens a device."""
import importlib.util
import json
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOLS = os.path.join(ROOT, "tools")

# the first four lines of profiles/static_bench.txt as tools/bench_static.py wrote them before the driver moved into video_bench.py
STATIC_RECORD_START = (
    "Blocks that do not change of the streamed video path (ssm_static_paste_fwd, --static; DESIGN 3.12).\n"
    "One MI355X, the default precision, synthetic weights and frames.  Tool: tools/bench_static.py (each step a process under its own time limit).\n"
    "Nothing is asserted; with synthetic weights nothing can be said about quality.\n"
    "\n"
    "== kernel_bytes: `python tools/bench_static.py --only kernel_bytes` (limit 180 s, exit status 0) ==\n")

# per tool: the record under profiles/ that --out defaults to, and every integer flag with its default, as each tool's own main() had them
# before the parser moved into video_bench.py (bench_shutter_hdr times no whole runs: no --runs, and 5 windows)
COMMON = {"iters": 20, "windows": 7, "runs": 3}
TOOL_ARGS = {"bench_active": ("active_bench.txt", COMMON), "bench_cuts": ("scene_cut_bench.txt", {**COMMON, "frames": 41}),
         "bench_dedup": ("dedup_bench.txt", COMMON), "bench_detelecine": ("detelecine_bench.txt", COMMON),
         "bench_field_order": ("field_order_bench.txt", COMMON), "bench_fields": ("fields_bench.txt", COMMON),
         "bench_score": ("video_score_bench.txt", COMMON), "bench_shutter": ("shutter_bench.txt", {**COMMON, "frames": 41}),
         "bench_shutter_hdr": ("shutter_hdr_bench.txt", {"iters": 20, "windows": 5, "rounds": 3}),
         "bench_shutter_light": ("shutter_light_bench.txt", {**COMMON, "frames": 41}),
         "bench_shutter_window": ("shutter_window_bench.txt", {**COMMON, "frames": 41}), "bench_ssim": ("video_ssim_bench.txt", COMMON),
         "bench_static": ("static_bench.txt", COMMON), "bench_tiled": ("tiled_bench.txt", {**COMMON, "passes": 12})}

STAND_IN = '''import sys
import time

sys.path.insert(0, %(tools)r)
from video_bench import drive, parser, run_only

STEPS = %(steps)r


def run_step(step, args):
    if step == "b":
        sys.exit(3)
    if step == "c":
        open(%(marker)r, "w").close()
    if step == "sleeps":
        time.sleep(30)
    return {"args": {k: v for k, v in vars(args).items() if k != "out"}}


def main():
    args = parser("stand_in.txt", STEPS, frames=41).parse_args()
    if args.only:
        return run_only(args.only, lambda: run_step(args.only, args))
    return drive(__file__, "Head, line 1.\\nLine 2.\\n", STEPS, args)


sys.exit(main())
'''


@pytest.fixture()
def vb():
    """tools/video_bench.py as a module, with sys.path as it was before its path setup."""
    path = list(sys.path)
    spec = importlib.util.spec_from_file_location("video_bench_under_test", os.path.join(TOOLS, "video_bench.py"))
    mod = importlib.util.module_from_spec(spec)
    try:
        spec.loader.exec_module(mod)
    finally:
        sys.path[:] = path
    return mod


def run_stand_in(tmp_path, steps, *flags):
    tool, out, marker = tmp_path / "stand_in.py", tmp_path / "record.txt", tmp_path / "c_ran"
    tool.write_text(STAND_IN % {"tools": TOOLS, "steps": steps, "marker": str(marker)})
    r = subprocess.run([sys.executable, str(tool), "--out", str(out)] + list(flags), stdout=subprocess.PIPE, text=True, timeout=60)
    return r, out.read_text(), marker


def section(step, limit, status):
    return "\n== %s: `python tools/stand_in.py --only %s` (limit %d s, exit status %d) ==\n" % (step, step, limit, status)


def test_driver_stops_at_the_first_failure_and_hands_every_flag_on(tmp_path):
    r, record, marker = run_stand_in(tmp_path, (("a", 20), ("b", 20), ("c", 20)), "--iters", "5", "--windows", "3", "--runs", "2", "--frames", "9")
    assert r.returncode == 3 and not marker.exists()
    a = {"a": {"args": {"only": "a", "iters": 5, "windows": 3, "runs": 2, "frames": 9}}}          # what the child parsed
    assert record == "Head, line 1.\nLine 2.\n" + section("a", 20, 0) + json.dumps(a, indent=1) + "\n" + section("b", 20, 3)
    assert r.stdout.splitlines() == ["a: exit status 0 " + json.dumps(a), "b: exit status 3 "]


def test_driver_passes_the_defaults_when_no_flag_is_given(tmp_path):
    r, record, _ = run_stand_in(tmp_path, (("a", 20),))
    assert r.returncode == 0
    assert json.loads(record.split(" ==\n", 1)[1]) == {"a": {"args": {"only": "a", "iters": 20, "windows": 7, "runs": 3, "frames": 41}}}


def test_driver_ends_a_step_at_its_limit_and_starts_nothing_after(tmp_path):
    r, record, marker = run_stand_in(tmp_path, (("sleeps", 1), ("c", 20)))
    assert r.returncode == 124 and not marker.exists()
    assert record == "Head, line 1.\nLine 2.\n" + section("sleeps", 1, 124)


def test_record_starts_as_bench_static_wrote_it():
    head = subprocess.run([sys.executable, "-c", "import sys; sys.path.insert(0, %r); import bench_static; sys.stdout.write(bench_static.HEAD)" % TOOLS],
                          stdout=subprocess.PIPE, text=True, check=True).stdout
    line = section("kernel_bytes", 180, 0).replace("stand_in.py", "bench_static.py")
    assert head + line == STATIC_RECORD_START
    with open(os.path.join(ROOT, "profiles", "static_bench.txt")) as f:
        assert f.read().startswith(STATIC_RECORD_START)


def test_parser_takes_a_flag_away_and_replaces_a_default(vb):
    args = vb.parser("x.txt", (("kernel", 1),), windows=5, runs=None, rounds=3).parse_args([])
    assert vars(args) == {"only": None, "out": os.path.join(ROOT, "profiles", "x.txt"), "iters": 20, "windows": 5, "rounds": 3}


def test_summaries_on_a_fake_clock(vb, monkeypatch):
    assert vb.per_s(10, [1.0, 2.0, 4.0]) == {"median": 5.0, "min": 2.5, "max": 10.0}
    assert vb.per_s(3, [7.0]) == {"median": 0.43, "min": 0.43, "max": 0.43}
    calls, seen = {"x": [], "y": []}, []
    clock = {"x": iter([0.30004, 0.10006, 0.2]), "y": iter([3.0, 1.0, 2.0])}

    def window_ms(fn, iters):          # the name of the callable it was given, and the next reading of that callable's clock
        name = fn()
        seen.append((name, iters, {k: len(v) for k, v in calls.items()}))
        return next(clock[name])

    monkeypatch.setattr(vb, "window_ms", window_ms)
    fns = {k: (lambda k=k: calls[k].append(1) or k) for k in calls}
    ms = vb.alternated_ms(fns, 4, 3)
    assert ms == {"x": {"median": 0.2, "min": 0.1001, "max": 0.3}, "y": {"median": 2.0, "min": 1.0, "max": 3.0}}
    assert [s[:2] for s in seen] == [("x", 4), ("y", 4)] * 3          # a round times every call once, in order
    assert seen[0][2] == {"x": 6, "y": 5}          # 5 untimed calls of EVERY callable before the first window
    clock["x"] = iter([5.0, 1.0, 2.0, 9.0])
    assert vb.call_ms(fns["x"], 2, 4) == 3.5          # the median of its windows, not rounded


def test_timed_legs_discards_the_warm_up_turns_and_calls_the_hook_every_turn(vb):
    log = []
    clock = iter(range(1, 100))

    def run(leg):
        log.append(leg)
        return next(clock)

    assert vb.timed_legs(("p", "q"), run, 2) == {"p": [3, 5], "q": [4, 6]}          # one turn discarded
    assert log == ["p", "q"] * 3
    del log[:]
    assert vb.timed_legs(("p", "q"), run, 1, warmup=2, between=log.append) == {"p": [11], "q": [12]}
    assert log == [0, "p", "q", 1, "p", "q", 2, "p", "q"]


@pytest.mark.parametrize("tool", sorted(TOOL_ARGS))
def test_tool_answers_help(tool):
    r = subprocess.run([sys.executable, os.path.join(TOOLS, tool + ".py"), "--help"], stdout=subprocess.PIPE, text=True, timeout=60)
    assert r.returncode == 0
    flags = set(re.findall(r"--[a-z_]+", r.stdout))
    assert flags == {"--help", "--only", "--out"} | {"--" + k for k in TOOL_ARGS[tool][1]}


def test_every_tool_keeps_its_defaults_and_imports_no_torch_before_its_step_runs():
    """Each tool's main() with no flag given, its `drive` replaced by one that prints what it was handed: the default --out and every
    default it would pass on to its steps, and its STEPS' names as the --only choices."""
    code = ("import json, sys; sys.path.insert(0, %r); sys.argv = sys.argv[:1]\n"
            "got = {}\n"
            "for name in %r:\n"
            "    tool = __import__(name)\n"
            "    tool.drive = lambda f, head, steps, args: got.update({name: [f, head, [s for s, _ in steps], vars(args)]}) or 0\n"
            "    assert tool.main() == 0 and got[name][2] == [s for s, _ in tool.STEPS]\n"
            "assert 'torch' not in sys.modules\n"
            "print(json.dumps(got))" % (TOOLS, sorted(TOOL_ARGS)))
    got = json.loads(subprocess.run([sys.executable, "-c", code], stdout=subprocess.PIPE, text=True, check=True, timeout=60).stdout)
    for name, (record, ints) in TOOL_ARGS.items():
        tool_file, head, steps, args = got[name]
        assert os.path.samefile(tool_file, os.path.join(TOOLS, name + ".py")) and "tools/%s.py" % name in head and head.endswith("\n")
        assert args == {"only": None, "out": os.path.join(ROOT, "profiles", record), **ints}, name
        assert list(args)[2:] == list(ints), name          # the order in which the driver hands them on
