"""What the streamed-video benchmarks (tools/bench_*.py of DESIGN 3.12 and 3.15) share: the import path, the copy ceiling, the event
timers, the synthetic model and clip, the alternating loop of whole runs, and the driver that runs each step of a tool as a child process
under its own `timeout`.  A module to import, not a tool: nothing here touches the GPU when it is imported, and torch is imported by the
functions that need it.  A new benchmark supplies STEPS ((step, time limit in seconds), ...), the head of its record and its step
functions, and a main() of three lines:
    args = parser("NAME_bench.txt", STEPS).parse_args()
    if args.only:
        return run_only(args.only, lambda: run_step(args.only, args))
    return drive(__file__, HEAD, STEPS, args)"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "superslomo-videointerpolation-pytorch_amd")
for p in (ROOT, PKG, os.path.join(PKG, "scripts"), os.path.join(ROOT, "tools")):          # a tool may put another package in front later
    sys.path.insert(0, p)

COPY_CEILING_BYTES_PER_S = 6.29e12          # the device-to-device copy of DESIGN 3.12: what a kernel that touches every byte once is held against


# ---- event timers ------------------------------------------------------------------------------------------------------------------
def window_ms(fn, iters):
    """ms per call of `iters` back-to-back calls between two device events."""
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def alternated_windows(calls, iters, windows):
    """{name: [ms per call, window by window]}: 5 untimed calls of each, then `windows` rounds, each timing every call once in turn."""
    for fn in calls.values():
        for _ in range(5):
            fn()
    out = {k: [] for k in calls}
    for _ in range(windows):
        for k, fn in calls.items():
            out[k].append(window_ms(fn, iters))
    return out


def alternated_ms(calls, iters, windows):
    """{name: {median, min, max}} of alternated_windows."""
    return {k: {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}
            for k, v in alternated_windows(calls, iters, windows).items()}


def call_ms(fn, iters, windows):
    """Median ms per call of one callable: 5 untimed calls, then `windows` windows."""
    for _ in range(5):
        fn()
    return statistics.median([window_ms(fn, iters) for _ in range(windows)])


# ---- the synthetic model and clip --------------------------------------------------------------------------------------------------
def synthetic_model(dev):
    """(model, cfg): FullModel of superslomo_original.ini with the synthetic weights, on `dev`, in eval mode."""
    from models.superslomo_r import FullModel
    from ssm_amd.config import load_config, synthetic_weight_overrides
    from ssm_amd.weights import synthetic_state_dict
    cfg = load_config("superslomo_original.ini", synthetic_weight_overrides())
    model = FullModel(cfg)
    model.stage1_model.load_state_dict(synthetic_state_dict(1))
    model.stage2_model.load_state_dict(synthetic_state_dict(2))
    return model.to(dev).eval(), cfg


def synthetic_payloads(n_frames, h, w, dev, cfg, seed=42):
    """[n_frames, frame_bytes] uint8 numpy: synthetic_frames_u8 as 420jpeg payloads, limited range, default_matrix(h), converted on the
    GPU 8 frames at a time."""
    import torch
    from ssm_amd import frames as F
    from ssm_amd import video as V
    from ssm_amd.weights import synthetic_frames_u8
    rgb = synthetic_frames_u8(n_frames, h, w, seed=seed).permute(0, 2, 3, 1).contiguous()
    return torch.cat([V.frames_to_yuv(F.frames_from_u8(rgb[i:i + 8].to(dev), cfg, True), h, w, V.CENTRED, V.default_matrix(h), V.LIMITED, cfg).cpu()
                      for i in range(0, n_frames, 8)]).numpy()


def write_y4m(path, payloads, w, h, rate, chroma="420jpeg", **kw):
    from ssm_amd import video as V
    with V.Y4MWriter(path, w, h, rate=rate, aspect=(1, 1), chroma=chroma, **kw) as wr:
        for p in payloads:
            wr.write_frame(p)


# ---- whole runs, legs in turns -----------------------------------------------------------------------------------------------------
def timed_legs(legs, run, runs, warmup=1, between=None):
    """{leg: [seconds of each timed run]}.  `warmup + runs` turns; a turn calls `between(turn)`, then `run(leg)` for every leg in order.
    `run` returns the seconds it measured - where its clock starts and stops is the tool's business - and the first `warmup` turns
    (plans, the pinned buffers' first touch, the first run on shared streams) are not kept."""
    secs = {k: [] for k in legs}
    for turn in range(warmup + runs):
        if between:
            between(turn)
        for k in legs:
            dt = run(k)
            if turn >= warmup:
                secs[k].append(dt)
    return secs


def share_streams(vis):
    """A `between` for timed_legs(warmup=2): at turn 1, once turn 0 has built every pipeline, the VideoInterpolators after the first
    get the first one's HIP streams.  Which hardware queues a pipeline's streams are dealt moves a leg by more than 10 %,
    and the legs never run at the same time."""
    def between(turn):
        if turn == 1:
            for vi in vis[1:]:
                vi._pipe[1].streams = vis[0]._pipe[1].streams
    return between


def per_s(count, seconds):
    v = [count / t for t in seconds]
    return {"median": round(statistics.median(v), 2), "min": round(min(v), 2), "max": round(max(v), 2)}


# ---- the step driver ---------------------------------------------------------------------------------------------------------------
def parser(out_name, steps, **int_flags):
    """--only, --out (profiles/`out_name`), --iters 20, --windows 7, --runs 3 and the tool's own integer flags (name=default).  A default
    given for one of the three replaces it; None takes the flag away."""
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", choices=[s for s, _ in steps], default=None, help="run this step in this process (what the driver starts)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", out_name))
    for name, default in {"iters": 20, "windows": 7, "runs": 3, **int_flags}.items():
        if default is not None:
            ap.add_argument("--" + name, type=int, default=default)
    return ap


def run_only(step, fn):
    """The --only branch: the step runs in this process and prints its record as one JSON line."""
    print(json.dumps({step: fn()}))
    return 0


def drive(tool_file, head, steps, args):
    """Writes `head` to args.out, then runs every step as `timeout -k 10 LIMIT python TOOL --only STEP` with every other flag of `args`
    passed on, and appends a section per step with the step's record.  Returns the first non-zero exit status - a failure, a fault or a
    time limit - and starts nothing after it: nothing more runs on a GPU that a step may have left in trouble."""
    name = os.path.basename(tool_file)
    flags = [x for k, v in vars(args).items() if k not in ("only", "out") for x in ("--" + k, str(v))]
    with open(args.out, "w") as f:
        f.write(head)
    for step, limit in steps:
        r = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(tool_file), "--only", step] + flags,
                           stdout=subprocess.PIPE, text=True)
        line = r.stdout.strip().splitlines()[-1] if r.stdout.strip() else ""
        with open(args.out, "a") as f:
            f.write("\n== %s: `python tools/%s --only %s` (limit %d s, exit status %d) ==\n" % (step, name, step, limit, r.returncode))
            if r.returncode == 0:
                f.write(json.dumps(json.loads(line), indent=1) + "\n")
        print("%s: exit status %d %s" % (step, r.returncode, line), flush=True)
        if r.returncode != 0:
            return r.returncode
    return 0
