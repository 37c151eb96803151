"""Forward-backward flow consistency without a GPU: the numpy yardstick (ssm_amd.flow_eval.flow_consistency_host) against the definition
of include/ssm_hip.h written out pixel by pixel in np.float32 scalars, closed forms, the strict edge of the threshold, FlowCheck, the
option's parser, the refused option combinations, and the entry point's argument refusals (the library loads without a device)."""
import os
import sys
from fractions import Fraction as Fr

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

f32 = np.float32


def FE():
    from ssm_amd import flow_eval
    return flow_eval


def by_pixel(flow4, top, left, H, W, alpha, beta):
    """The definition, one np.float32 operation per step, pixel by pixel: (record [N,2,4], mask [N,2,H,W])."""
    alpha, beta = f32(alpha), f32(beta)
    n = flow4.shape[0]
    record, mask = np.zeros((n, 2, 4), np.float64), np.zeros((n, 2, H, W), np.uint8)
    for k in range(n):
        crop = flow4[k, :, top:top + H, left:left + W]
        for d in (0, 1):
            F, G = crop[2 * d:2 * d + 2], crop[2 - 2 * d:4 - 2 * d]
            for y in range(H):
                for x in range(W):
                    u, v = F[0, y, x], F[1, y, x]
                    px, py = f32(x) + u, f32(y) + v
                    if not (px >= 0 and px <= f32(W - 1) and py >= 0 and py <= f32(H - 1)):
                        mask[k, d, y, x] = 2
                        record[k, d, 2] += 1
                        continue
                    x0, y0 = np.floor(px), np.floor(py)
                    fx, fy = px - x0, py - y0
                    xi0, yi0 = int(x0), int(y0)
                    xi1, yi1 = min(xi0 + 1, W - 1), min(yi0 + 1, H - 1)
                    s = []
                    for g in G:
                        a = g[yi0, xi0] + fx * (g[yi0, xi1] - g[yi0, xi0])
                        b = g[yi1, xi0] + fx * (g[yi1, xi1] - g[yi1, xi0])
                        s.append(a + fy * (b - a))
                    rx, ry = u + s[0], v + s[1]
                    e2 = rx * rx + ry * ry
                    m2 = ((u * u + v * v) + s[0] * s[0]) + s[1] * s[1]
                    assert all(type(z) is f32 for z in (px, fx, s[0], e2, m2, alpha * m2 + beta))
                    bad = bool(e2 > alpha * m2 + beta)
                    mask[k, d, y, x] = 1 if bad else 0
                    record[k, d, 0] += 1
                    record[k, d, 1] += bad
                    record[k, d, 3] += float(np.sqrt(e2))
    return record, mask


def fields(n, hv, wv, seed, reach=3.0):
    rng = np.random.RandomState(seed)
    c = rng.uniform(-reach, reach, size=(n, 2, 1, 1))
    return np.concatenate([c + rng.uniform(-0.7, 0.7, size=(n, 2, hv, wv)), -c + rng.uniform(-0.7, 0.7, size=(n, 2, hv, wv))], 1).astype(f32)


@pytest.mark.parametrize("h,w", [(5, 7), (9, 4)])
def test_array_yardstick_equals_the_loop(h, w):
    fe = FE()
    flow = fields(2, h + 3, w + 4, seed=10 * h + w)
    flow[:, :, :1], flow[:, :, h + 1:], flow[:, :, :, :2], flow[:, :, :, w + 2:] = np.nan, np.nan, np.nan, np.nan          # the canvas around the crop
    want, want_mask = by_pixel(flow, 1, 2, h, w, fe.FLOW_ALPHA, fe.FLOW_BETA)
    got, mask = fe.flow_consistency_host(flow, 1, 2, h, w, fe.FLOW_ALPHA, fe.FLOW_BETA)
    assert np.array_equal(mask, want_mask) and np.array_equal(got[..., :3], want[..., :3])
    assert all((want_mask == s).any() for s in (0, 1, 2)), "every state occurs"
    assert np.allclose(got[..., 3], want[..., 3], rtol=1e-12, atol=0) and not np.isnan(got).any()
    assert (got[..., 0] + got[..., 2] == h * w).all()


def constant(h, w, f01, f10):
    x = np.empty((1, 4, h, w), f32)
    x[0, 0], x[0, 1], x[0, 2], x[0, 3] = f01[0], f01[1], f10[0], f10[1]
    return x


# 6 x 9.  F01 = (+2, -1): x + 2 <= 8 keeps 7 columns, y - 1 >= 0 keeps 5 rows: 35 stay, 19 leave; F10 = (-2, +1) the mirror image.
# (0.5, 0.25): x + 0.5 <= 8 keeps 8 columns, y + 0.25 <= 5 keeps 5 rows: 40 stay, 14 leave; (-0.5, -0.25): x >= 1 and y >= 1, the same.
@pytest.mark.parametrize("f,stay", [((2.0, -1.0), (35, 35)), ((0.5, 0.25), (40, 40))])
def test_closed_form_constant_fields(f, stay):
    h, w = 6, 9
    got, mask = FE().flow_consistency_host(constant(h, w, f, (-f[0], -f[1])), 0, 0, h, w, 0.01, 0.5)
    for d in (0, 1):
        assert got[0, d].tolist() == [stay[d], 0, h * w - stay[d], 0.0]
        assert (mask[0, d] == 2).sum() == h * w - stay[d] and (mask[0, d] == 1).sum() == 0
    assert not mask[0, 0, 1:, :7].any() and (mask[0, 0, 0] == 2).all() if f == (2.0, -1.0) else True


def test_the_strict_edge():
    """alpha = 0, F01 = (2, 0), F10 = (-1, 0): e2 = 1 wherever a pixel is judged; `>` is strict."""
    h, w = 6, 9
    x = constant(h, w, (2.0, 0.0), (-1.0, 0.0))
    at, _ = FE().flow_consistency_host(x, 0, 0, h, w, 0.0, 1.0)
    below, _ = FE().flow_consistency_host(x, 0, 0, h, w, 0.0, np.nextafter(f32(1), f32(0)))
    assert at[0, :, 0].tolist() == [h * (w - 2), h * (w - 1)] == below[0, :, 0].tolist()
    assert at[0, :, 1].tolist() == [0, 0] and below[0, :, 1].tolist() == below[0, :, 0].tolist()
    assert at[0, :, 3].tolist() == [float(h * (w - 2)), float(h * (w - 1))]


def test_nan_and_inf_flows_leave():
    h, w = 5, 6
    x = constant(h, w, (0.0, 0.0), (0.0, 0.0))
    x[0, 0, 1, 1], x[0, 1, 2, 2], x[0, 0, 3, 3], x[0, 3, 4, 4] = np.nan, np.inf, -np.inf, np.nan
    got, mask = FE().flow_consistency_host(x, 0, 0, h, w, 0.01, 0.5)
    assert mask[0, 0, 1, 1] == mask[0, 0, 2, 2] == mask[0, 0, 3, 3] == mask[0, 1, 4, 4] == 2
    assert got[0, :, 2].tolist() == [3, 1] and got[0, :, 0].tolist() == [h * w - 3, h * w - 1]


def test_flow_check_record():
    fe = FE()
    c = fe.FlowCheck.of([[10, 3, 2, 4.5], [8, 4, 4, 3.5]])
    assert c == fe.FlowCheck((10, 8), (3, 4), (2, 4), (4.5, 3.5))
    assert c.share(0) == Fr(3, 10) and c.share(1) == Fr(1, 2) and c.score == Fr(1, 2) and c.mean_residual == 8.0 / 18
    none = fe.FlowCheck.of([[0, 0, 12, 0.0], [12, 0, 0, 0.0]])
    assert none.share(0) == 1 and none.share(1) == 0 and none.score == 1, "nothing judged vouches for nothing"
    assert fe.FlowCheck.of(np.zeros((2, 4))).mean_residual == 0.0


def test_parser():
    p = FE().parse_flow_check
    assert p(True) == (None, None, None)
    assert p("0.2") == (Fr(1, 5), None, None) == p(Fr(1, 5)) == p(" 1/5 ")
    assert p("1/5:0.01:0.5") == (Fr(1, 5), Fr(1, 100), Fr(1, 2)) == p((Fr(1, 5), "0.01", "1/2"))
    assert p("2") == (Fr(2), None, None) and p(0) == (Fr(0), None, None)
    assert p("0.2", alpha="0.02") == (Fr(1, 5), Fr(1, 50), None) and p(True, beta=1) == (None, None, Fr(1))
    for bad in ("", "x", "0.2:0.01", "0.2:0.01:0.5:1", "1/0", "-0.1", "0.2:-1:0.5", "0.2:0.01:nan", False, None, (1, 2)):
        with pytest.raises(ValueError, match="flow check") as e:
            p(bad)
        assert repr(bad) in str(e.value) or repr(str(bad).split(":")[-1]) in str(e.value) or "-1" in str(e.value), str(e.value)


class _Model:          # what the constructor looks at ahead of any GPU work
    recurrent = False


class _Recurrent:
    recurrent = True


class _NoWriter:
    def __getattr__(self, name):
        raise AssertionError("the writer was touched: %s" % name)


def test_refused_combinations_raise_before_a_writer_is_touched(tmp_path):
    from ssm_amd import video as V
    from ssm_amd.config import load_config, synthetic_weight_overrides
    cfg = load_config("superslomo_original.ini", synthetic_weight_overrides())
    for name, kw, model in (("shutter", dict(shutter=Fr(1, 2), speed=1), _Model()), ("deinterlace", dict(deinterlace="tff"), _Model()),
                            ("dedup", dict(dedup=True), _Model()), ("flow_scale=2", dict(flow_scale=2), _Model()),
                            ("tile", dict(tile=(64, 64), halo=32, blend=0), _Model()), ("a recurrent model", {}, _Recurrent())):
        with pytest.raises(ValueError, match="flow_check together with %s is not available" % name):
            V.VideoInterpolator(model, cfg, flow_check=Fr(1, 5), **kw)
    with pytest.raises(ValueError, match="flow check"):
        V.VideoInterpolator(_Model(), cfg, flow_check="often")
    with pytest.raises(ValueError, match="give flow_check"):
        V.VideoInterpolator(_Model(), cfg, flow_alpha=0.02)
    vi = V.VideoInterpolator(_Model(), cfg, flow_check="1/5", flow_beta="1/4", scene_cut="1/10", static=0, target_rate=(60, 1))
    assert vi.flow_check == (Fr(1, 5), 0.01, 0.25) and vi.flow_checks == [] and vi.flow_failed == []
    assert V.VideoInterpolator(_Model(), cfg, flow_check=True).flow_check == (None, 0.01, 0.5)
    assert V.VideoInterpolator(_Model(), cfg).flow_check is None
    # the command line refuses the same by name, in its argument parser: no reader, no writer, no model
    import interpolate_video
    src, dst = str(tmp_path / "in.y4m"), str(tmp_path / "out.y4m")
    base = ["-c", "x.ini", "--expt", "t", "--log", str(tmp_path / "log"), "--input", src, "--output", dst]
    for flags, name in ((["--shutter", "180", "--speed", "1"], "--shutter"), (["--deinterlace", "tff"], "--deinterlace"), (["--dedup"], "--dedup"),
                        (["--flow_scale", "2"], "--flow_scale 2"), (["--tile", "64x64"], "--tile")):
        with pytest.raises(SystemExit):
            interpolate_video.getargs(base + ["--flow_check", "0.2"] + flags)
    with pytest.raises(SystemExit):
        interpolate_video.getargs(base + ["--flow_check", "often"])
    assert interpolate_video.getargs(base + ["--flow_check"]).flow_check == (None, None, None)
    assert interpolate_video.getargs(base + ["--flow_check", "1/5:0.02:1"]).flow_check == (Fr(1, 5), Fr(1, 50), Fr(1))
    assert interpolate_video.getargs(base).flow_check is None
    assert not os.path.exists(dst)


def test_log_lines():
    import interpolate_video
    fe = FE()
    checks = [(0, fe.FlowCheck((10, 10), (1, 2), (0, 0), (5.0, 5.0))), (1, fe.FlowCheck((10, 10), (5, 0), (0, 0), (20.0, 0.0))),
              (2, fe.FlowCheck((10, 10), (0, 0), (0, 0), (0.0, 0.0)))]
    lines = interpolate_video.flow_check_lines(checks, checks[1:2], (Fr(2, 5), 0.01, 0.5))
    assert len(lines) == 2 and "3 pairs scored" in lines[0] and "at least 0.000000, median 0.200000, at most 0.500000" in lines[0]
    assert "largest mean residual 1.0000 px" in lines[0] and "1 pairs fell back" in lines[0]
    assert "flow check failed between input frames 1 and 2: score 1/2 = 0.500000 (threshold 2/5)" in lines[1]
    assert interpolate_video.flow_check_lines([], [], (None, 0.01, 0.5)) == ["flow check: alpha = 0.01, beta = 0.5, no pair ran"]


def test_entry_point_refuses_bad_arguments():
    """As tests/test_cabi_cpu.py: bad arguments are refused on the host with a message, no launch."""
    from ssm_amd import hipbind as hb
    lib = hb.load()
    good = hb.SsmView(64, 0, 0, 8)

    def call(view=good, n=1, h=4, w=4, top=0, left=0, ws=64, out=64):
        return lib.ssm_flow_consistency_fwd(view, n, h, w, top, left, 0.01, 0.5, ws, out, None, None), lib.ssm_last_error_string().decode()

    for kw, text in ((dict(view=hb.SsmView(None, 0, 0, 8)), "null pointer (flow)"), (dict(ws=None), "null pointer"), (dict(out=None), "null pointer"),
                     (dict(n=0), "N = 0"), (dict(n=-1), "N = -1"), (dict(h=0), "0x4 field"), (dict(w=-2), "4x-2 field"),
                     (dict(top=-1), "crop origin (-1, 0) is negative"), (dict(left=5), "row stride 8 is shorter than left + W = 9"),
                     (dict(w=9), "row stride 8 is shorter than left + W = 9"), (dict(ws=68), "8-byte aligned")):
        rc, msg = call(**kw)
        assert rc == -1 and text in msg and msg.startswith("flow_consistency"), (kw, msg)
    assert lib.ssm_flow_consistency_workspace_bytes(0, 4, 4) == 0 == lib.ssm_flow_consistency_workspace_bytes(1, 4, -1)
    assert lib.ssm_flow_consistency_workspace_bytes(1, 1, 1) == 64 and lib.ssm_flow_consistency_workspace_bytes(3, 50, 200) == 3 * 5 * 64
