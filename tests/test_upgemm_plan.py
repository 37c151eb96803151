"""A stage-2 plan with its inner decoder levels (conv7a, conv8a, conv9a) in the low-res GEMM form (csrc/ssm_upgemm.hip,
$SSM_UPGEMM) against the same plan without it: every decoder tensor, the frames, and the hoisted against the un-hoisted plan
(scripts/models/flow_computation.py:244-247 is the step the form evaluates)."""
import pytest
import torch

pytestmark = pytest.mark.gpu
H, W = 64, 96
DECODER_T = ("t7a", "c7", "t8a", "c8", "t9a", "c9", "t10a", "c10", "t11a", "c11", "tf")
FRAME_BAR = 2e-4          # tests/test_hip_model.py tol_frame at <= 352 px, against the oracle


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def runs(dev):
    """(frames, decoder tensors, algorithms) of the 64x96 pair engine for (upgemm, hoist) in on/off x on/off, and the oracle's frames."""
    import ssm_amd.engine as E
    from oracle import ssm_oracle as O
    from ssm_amd.weights import synthetic_frames, synthetic_state_dict
    sd1c, sd2c = synthetic_state_dict(1, True), synthetic_state_dict(2, True)
    sd1 = {k: v.to(dev) for k, v in sd1c.items()}
    sd2 = {k: v.to(dev) for k, v in sd2c.items()}
    img6 = synthetic_frames(2, H, W, seed=61).reshape(1, 6, H, W)
    ts = [0.125, 0.5, 0.875]
    out = {"oracle": torch.cat(O.interpolate_pair(sd1c, sd2c, img6, ts), 0)}
    for up in ("conv7a,conv8a,conv9a", "0"):
        for hoist in (True, False):
            old = E.UPGEMM, E.HOIST_PAIR_PARTS
            E.UPGEMM, E.HOIST_PAIR_PARTS = up, hoist
            try:
                eng = E.PairEngine(sd1, sd2, 1, 3, H, W, dev, True, "f32w")
            finally:
                E.UPGEMM, E.HOIST_PAIR_PARTS = old
            assert (eng.s2.hoist is not None) == hoist
            frames = eng.run(img6.to(dev), torch.tensor(ts, device=dev), want_aux=True).clone().cpu()
            out[up != "0", hoist] = (frames, {n: eng.s2.t[n].to_nchw().cpu() for n in DECODER_T},
                                     {n: eng.s2.pk[n].algo for n in ("conv7a", "conv8a", "conv9a", "conv10a")})
    return out


def _rel(a, b):
    return float((a - b).abs().max()) / float(b.abs().max())


@pytest.mark.parametrize("hoist", [True, False])
def test_selected_layers_run_in_the_form_and_every_decoder_tensor_agrees(runs, hoist):
    (_, ta, algo_a), (_, tb, algo_b) = runs[True, hoist], runs[False, hoist]
    assert [algo_a[n] for n in ("conv7a", "conv8a", "conv9a")] == ["upgemm"] * 3 and algo_a["conv10a"] != "upgemm"
    assert "upgemm" not in algo_b.values()
    for n in DECODER_T:
        r = _rel(ta[n], tb[n])
        print("hoist %s %s: %.3e of max|tensor|" % (hoist, n, r))
        assert r < 5e-5, "%s: %.3e of max|tensor|" % (n, r)


def test_frames_meet_the_oracle_bar(runs):
    for key in ((True, True), (True, False), (False, True)):
        e = float((runs[key][0] - runs["oracle"]).abs().max())
        print("upgemm %s hoist %s: frames %.3e from the oracle" % (key + (e,)))
        assert e < FRAME_BAR, (key, e)


def test_hoisted_plan_equals_the_unhoisted_one(runs):
    (fa, ta, _), (fb, tb, _) = runs[True, True], runs[True, False]
    for n in DECODER_T:
        r = _rel(ta[n], tb[n])
        print("hoisted vs per-t %s: %.3e of max|tensor|" % (n, r))
        assert r < 5e-5, "%s: %.3e of max|tensor|" % (n, r)
    assert float((fa - fb).abs().max()) < FRAME_BAR
