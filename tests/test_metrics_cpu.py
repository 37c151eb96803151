"""No-GPU checks of the device metrics' host side: the sums -> (PSNR, SSIM, IE) assembly of ssm_amd.evaluation.metrics_from_sums
against the host metrics (psnr / ssim / interpolation_error), fed with the five per-frame sums computed in numpy, and the C entry
point's argument checks (refused before any launch)."""
import ctypes

import numpy as np
import pytest


def numpy_sums(t, o):
    """(SSE, IE sum, SSIM sum c0, c1, c2) of one uint8 HxWx3 pair: the record ssm_frame_metrics_fwd writes."""
    from scipy.ndimage import gaussian_filter
    d = t.astype(np.int64) - o.astype(np.int64)
    sse = float((d * d).sum())
    ie = float(np.sqrt((d * d).sum(axis=2).astype(np.float64)).sum())
    cov, c1, c2 = 121.0 / 120.0, (0.01 * 255.0) ** 2, (0.03 * 255.0) ** 2
    sums = []
    for c in range(3):
        x, y = t[..., c].astype(np.float64), o[..., c].astype(np.float64)
        g = lambda a: gaussian_filter(a, sigma=1.5, truncate=3.5, mode="reflect")  # noqa: E731
        ux, uy = g(x), g(y)
        vx, vy, vxy = cov * (g(x * x) - ux * ux), cov * (g(y * y) - uy * uy), cov * (g(x * y) - ux * uy)
        s = ((2 * ux * uy + c1) * (2 * vxy + c2)) / ((ux * ux + uy * uy + c1) * (vx + vy + c2))
        sums.append(float(s[5:-5, 5:-5].sum()))
    return [sse, ie] + sums


def pairs():
    rng = np.random.RandomState(3)
    for h, w in ((11, 11), (12, 37), (60, 90), (33, 130)):
        t = rng.randint(0, 256, (h, w, 3)).astype(np.uint8)
        yield t, rng.randint(0, 256, (h, w, 3)).astype(np.uint8)
        yield t, np.clip(t.astype(int) + rng.randint(-3, 4, t.shape), 0, 255).astype(np.uint8)
    flat = np.full((40, 50, 3), 117, np.uint8)
    yield flat, flat + 1
    yield flat, flat.copy()                                            # identical: PSNR inf, IE 0
    cb = ((np.indices((24, 31)).sum(0) % 2) * 255).astype(np.uint8)[..., None].repeat(3, 2)
    yield cb, 255 - cb


def test_sums_to_metrics_match_the_host_metrics():
    from ssm_amd.evaluation import interpolation_error, metrics_from_sums, psnr, ssim
    for t, o in pairs():
        h, w, _ = t.shape
        got = metrics_from_sums(np.array([numpy_sums(t, o)]), h, w)
        assert got.shape == (1, 3) and got.dtype == np.float64
        p, s, e = got[0]
        want_p = psnr(t, o)
        assert p == want_p or (np.isinf(p) and np.isinf(want_p)), (t.shape, p, want_p)
        assert abs(s - ssim(t, o)) <= 1e-9, (t.shape, s, ssim(t, o))
        want_e = interpolation_error(t, o)
        assert abs(e - want_e) <= 1e-12 * max(abs(want_e), 1e-300), (t.shape, e, want_e)
        if (t == o).all():
            assert np.isinf(p) and e == 0.0 and abs(s - 1.0) <= 1e-12


def test_psnr_assembly_is_bitwise_for_exact_sse():
    """A batch of records: PSNR per frame equals psnr() bit for bit (the SSE is an exact integer on both sides)."""
    from ssm_amd.evaluation import metrics_from_sums, psnr
    rng = np.random.RandomState(8)
    t = rng.randint(0, 256, (5, 23, 41, 3)).astype(np.uint8)
    o = rng.randint(0, 256, (5, 23, 41, 3)).astype(np.uint8)
    got = metrics_from_sums(np.array([numpy_sums(t[k], o[k]) for k in range(5)]), 23, 41)
    assert [float(v) for v in got[:, 0]] == [psnr(t[k], o[k]) for k in range(5)]


def test_entry_point_refuses_bad_arguments_before_launch():
    from ssm_amd import hipbind as hb
    lib = hb.load()
    nb = lib.ssm_frame_metrics_workspace_bytes(7, 720, 1280)
    assert nb == 7 * (1280 // 32) * (720 // 16) * 5 * 8               # one 5-double record per 32x16 tile
    assert lib.ssm_frame_metrics_workspace_bytes(1, 11, 11) == 5 * 8
    assert lib.ssm_frame_metrics_workspace_bytes(0, 64, 64) == 0
    fake = ctypes.c_void_p(16)                                        # never dereferenced: every call below fails its checks first
    cases = [((None, fake, 1, 64, 64, fake, 1 << 20, fake), b"null"),
             ((fake, fake, 0, 64, 64, fake, 1 << 20, fake), b"N = 0"),
             ((fake, fake, 1, 10, 64, fake, 1 << 20, fake), b"smaller than the 11x11"),
             ((fake, fake, 1, 64, 10, fake, 1 << 20, fake), b"smaller than the 11x11"),
             ((fake, fake, 2, 64, 64, fake, lib.ssm_frame_metrics_workspace_bytes(2, 64, 64) - 1, fake), b"workspace")]
    for args, msg in cases:
        assert lib.ssm_frame_metrics_fwd(*args, None) == -1
        assert msg in lib.ssm_last_error_string(), (args, lib.ssm_last_error_string())


def test_evaluator_rejects_an_unknown_metrics_mode():
    from ssm_amd.config import load_config
    from ssm_amd.evaluation import Evaluator
    cfg = load_config("superslomo_original.ini")
    with pytest.raises(AssertionError, match="metrics"):
        Evaluator(cfg, None, 60, 90, metrics="gpu")
