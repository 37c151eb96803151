"""Fixture of the optical-flow evaluation: tests/golden/flow_eval.npz.

    python tests/golden/make_golden_flow.py --reference <checkout of the reference repository>

Runs on the CPU.  Small seeded float32 flow fields go through the reference's own `compute_metrics`
(scripts/evaluate_optical_flow_results.py:18-28), `flo_utils.flow_to_image`, `make_color_wheel` and `write_flow`
(scripts/utils/flo_utils.py); only DATA is written (the inputs and what the reference returned for them), no reference source
travels.  `compute_metrics` lives in a script that parses arguments and builds a CUDA model when imported, so that one function's
definition is taken out of the file with `ast` at generation time and executed in a scratch namespace.  `flo_utils.flow_error`
does not run on the numpy used here, 2.2.6 (it indexes with a one-element list that holds a mask, flo_utils.py:113: "too many
indices"), so the records `m<k>_epe_mode1` are the generator's own evaluation of its evident definition - mean end-point error over the pixels
whose ground truth is known and not zero in both components, in float32 - and the fixture's `note` says so.
The reference's functions modify their arguments: they get copies.
"""
import argparse
import ast
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


def reference_compute_metrics(ref):
    path = os.path.join(ref, "scripts", "evaluate_optical_flow_results.py")
    tree = ast.parse(open(path).read(), path)
    fn = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "compute_metrics"]
    assert len(fn) == 1
    ns = {"np": np}
    exec(compile(ast.Module(body=fn, type_ignores=[]), path, "exec"), ns)
    return ns["compute_metrics"]


def smooth(rng, h, w, amp):
    """A smooth [h,w,2] float32 field: a few seeded sinusoids per component."""
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    out = np.zeros((h, w, 2))
    for c in range(2):
        for _ in range(4):
            fy, fx = rng.uniform(0.01, 0.12, 2)
            out[..., c] += rng.uniform(0.3, 1.0) * np.sin(fy * y + fx * x + rng.uniform(0, 2 * np.pi))
    return (amp * out / 2.0).astype(np.float32)


def clear_of_three(flow, gt, margin=1e-4):
    d = gt.astype(np.float64) - flow.astype(np.float64)
    err = np.sqrt((d * d).sum(axis=2))
    finite = err[np.isfinite(err)]
    return not (np.abs(finite - 3.0) < margin).any()


def metric_cases():
    """(flow, ground truth) pairs; no error within 1e-4 of 3 px (the seed moves on until that holds)."""
    cases = []
    for k, (h, w, kind) in enumerate(((54, 128, "smooth"), (37, 61, "ragged"), (54, 128, "zero region"), (54, 128, "unknown"))):
        seed = 100 * (k + 1)
        while True:
            rng = np.random.RandomState(seed)
            gt = smooth(rng, h, w, 9.0)
            flow = (gt + smooth(rng, h, w, 5.0)).astype(np.float32)
            if kind in ("zero region", "unknown"):
                gt[10:30, 20:70] = 0.0                      # identically zero ground truth: left out by mode 1
                gt[40:44, 5:9, 0] = 0.0                     # zero in ONE component: still counts
            if kind == "unknown":
                gt[5:9, 100:120, 0] = 1e9                   # unknown in u only
                gt[45:50, 60:64, 1] = -1e9                  # unknown in v only
                gt[12:14, 22:30] = 1e9                      # both
            if clear_of_three(flow, gt):
                break
            seed += 1
        cases.append((flow, gt, kind, seed))
    return cases


def colour_cases():
    rng = np.random.RandomState(7)
    out = [("smooth", smooth(rng, 54, 128, 7.0)), ("ragged", smooth(rng, 37, 61, 0.8))]
    z = smooth(rng, 54, 128, 3.0)
    z[20:40, 30:90] = 0.0
    z[5, 5] = (-0.0, 0.0)
    z[5, 6] = (2.0, -0.0)
    out.append(("zero region", z))
    u = smooth(rng, 54, 128, 4.0)
    u[3:6, 10:30, 0] = 1e9
    u[30:33, 50:52, 1] = -1e9
    u[40, 100] = (np.inf, 1.0)
    out.append(("unknown", u.copy()))
    u[8, 64, 0] = np.nan
    u[9, 65] = (np.nan, 1e9)                                # NaN in u, unknown in v: unknown wins
    u[47:49, 7:9, 1] = np.nan
    out.append(("unknown and nan", u))
    m = smooth(rng, 54, 128, 2.0)
    m[17, 93] = (11.0, -13.0)                               # the maximum radius at exactly one pixel
    out.append(("single maximum", m))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("SSM_REFERENCE"), required="SSM_REFERENCE" not in os.environ)
    args = ap.parse_args()
    sys.path.insert(0, os.path.join(args.reference, "scripts"))
    from utils import flo_utils as ref            # imports matplotlib.pyplot
    compute_metrics = reference_compute_metrics(args.reference)

    seen = {}
    inner = ref.compute_color

    def spy(u, v):
        seen["dtype"] = str(u.dtype)
        return inner(u, v)
    ref.compute_color = spy

    fix = {"numpy_version": np.array(np.__version__), "color_wheel": ref.make_color_wheel()}
    notes = ["m<k>_epe_mode1 is a restatement computed by the generator (flo_utils.flow_error does not run on this numpy), "
             "not a reference output; every other record is what the reference returned."]
    for k, (flow, gt, kind, seed) in enumerate(metric_cases()):
        epe, pct = compute_metrics(flow.copy()[None], gt.copy()[None])
        fix["m%d_flow" % k], fix["m%d_gt" % k] = flow, gt
        fix["m%d_epe" % k], fix["m%d_pct" % k] = np.asarray(epe), np.asarray(pct, dtype=np.float64)
        unknown = (np.abs(gt[..., 0]) > 1e7) | (np.abs(gt[..., 1]) > 1e7)
        counted = ~unknown & ((np.abs(gt[..., 0]) > 0) | (np.abs(gt[..., 1]) > 0))
        d = gt - flow
        err = np.sqrt(d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1])
        fix["m%d_epe_mode1" % k] = np.asarray(np.mean(err[counted]))
        fix["m%d_counted_mode1" % k] = np.asarray(int(counted.sum()))
        notes.append("m%d: %s, seed %d" % (k, kind, seed))
    for k, (kind, flow) in enumerate(colour_cases()):
        fix["c%d_flow" % k] = flow
        with np.errstate(invalid="ignore"):
            fix["c%d_image" % k] = ref.flow_to_image(flow.copy())
        fix["c%d_norm_dtype" % k] = np.array(seen["dtype"])
        notes.append("c%d: %s" % (k, kind))
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "f.flo")
        ref.write_flow(fix["m1_flow"].copy(), path)
        fix["m1_flo_bytes"] = np.frombuffer(open(path, "rb").read(), dtype=np.uint8)
    fix["norm_dtype"] = fix["c0_norm_dtype"]
    fix["note"] = np.array("\n".join(notes))
    out = os.path.join(HERE, "flow_eval.npz")
    np.savez_compressed(out, **fix)
    print("wrote %s (%d bytes, %d records)" % (out, os.path.getsize(out), len(fix)))


if __name__ == "__main__":
    main()
