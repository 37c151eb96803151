"""The frame-mix baseline of the hold-out score on the GPU: ssm_payload_mix_fwd against its numpy yardstick
(ssm_amd.video_score.payload_mix_host).  Integer arithmetic: the bytes must be EQUAL.  What the cases aim at: the division by multiply-shift
at small, odd and the largest den, rows that start at no particular alignment (the sample-by-sample path), the last piece of a row, a store
past `samples` or past row N, stride 0 on both operands (the scorer's call), and the refusals."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from video_clips import S, bits_of  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
# A workgroup takes a span of 16 KiB of a row: 16384 samples of one byte, 8192 of two (csrc/ssm_video.hip SPAN_BYTES).
SPAN = 16384
FILL = 0xa7
# samples of a row: 1; either side of a 16-byte piece; 4851 = a 45 x 71 4:2:0 frame, odd, so that rows 1, 3, ... of bytes start unaligned;
# either side of a span (of bytes; two spans of words)
SAMPLES = (1, 15, 16, 17, 4851, SPAN - 1, SPAN, SPAN + 1)


def rows(n, samples, sb, seed):
    rng = np.random.RandomState(seed + 13 * samples + sb)
    return rng.randint(0, 256, size=(n, samples * sb)).astype(np.uint8)


def mix(a, b, n, num0, step, den, sb, samples, slack=32):
    """The device op on numpy rows ([n or 1, samples * sb]; one row: stride 0) into a prefilled buffer of n + 1 rows with `slack` bytes
    after each: (the mixed rows, whether every byte outside them kept the prefill)."""
    s = S()
    row = samples * sb
    ta, tb = (torch.from_numpy(x).to(DEV) for x in (a, b))
    ta, tb = (t.expand(n, row) if t.shape[0] == 1 and n > 1 else t for t in (ta, tb))
    out = torch.full((n + 1, row + slack), FILL, dtype=torch.uint8, device=DEV)
    got = s.payload_mix(ta, tb, num0, step, den, bits_of(sb), out=out[:n], samples=samples)
    assert got.data_ptr() == out.data_ptr()
    host = out.cpu().numpy()
    clean = bool((host[:n, row:] == FILL).all() and (host[n] == FILL).all())
    return host[:n, :row], clean


@pytest.mark.parametrize("sb", [1, 2])
@pytest.mark.parametrize("den", [2, 8, 255, 65535])
@pytest.mark.parametrize("samples", SAMPLES)
def test_kernel_equals_its_yardstick(samples, den, sb):
    s = S()
    n = 3
    a, b = rows(n, samples, sb, 1), rows(n, samples, sb, 2)
    for num0, step in ((0, den // 2), (den, -(den // 2)), (1, 0)):          # k = 0, den // 2, 2 (den // 2); den downwards; 1 throughout
        got, clean = mix(a, b, n, num0, step, den, sb, samples)
        assert clean, "a byte after `samples`, or in the row after N, was written"
        assert np.array_equal(got, s.payload_mix_host(a, b, n, num0, step, den, bits_of(sb))), (num0, step)
    got, _ = mix(a, b, n, 0, 0, den, sb, samples)
    assert np.array_equal(got, a), "k = 0 reproduces a"
    got, _ = mix(a, b, n, den, 0, den, sb, samples)
    assert np.array_equal(got, b), "k = den reproduces b"


@pytest.mark.parametrize("sb", [1, 2])
@pytest.mark.parametrize("samples", [4851, 2 * SPAN + 16])
def test_the_scorers_call_one_pair_against_seven_positions(samples, sb):
    """Stride 0 on a and b, N = hold - 1 = 7, k = 1 .. 7 over 8."""
    s = S()
    a, b = rows(1, samples, sb, 3), rows(1, samples, sb, 4)
    got, clean = mix(a, b, 7, 1, 1, 8, sb, samples, slack=0 if samples % 16 == 0 else 6)
    assert clean and np.array_equal(got, s.payload_mix_host(a, b, 7, 1, 1, 8, bits_of(sb)))


def test_extremes_of_the_numerator():
    s = S()
    for sb, den in ((1, 255), (2, 65535), (2, 32768), (1, 256), (2, 3)):
        a = np.full((1, 64 * sb), 255, np.uint8)
        b = np.zeros((1, 64 * sb), np.uint8)
        n = 4
        ks = (0, 1, den // 2, den)
        for x, y in ((a, a), (a, b), (b, a)):
            for k in ks:
                got, clean = mix(x, y, n, k, 0, den, sb, 64)
                assert clean and np.array_equal(got, s.payload_mix_host(x, y, n, k, 0, den, bits_of(sb))), (sb, den, k)


def raw(a, b, sa, sb_, out, so, n, samples, sbytes, num0, step, den):
    from ssm_amd import hipbind as hb
    hb.check(hb.load().ssm_payload_mix_fwd(a, b, sa, sb_, out, so, n, samples, sbytes, num0, step, den, hb.stream_ptr()))


def test_refusals_by_name_and_out_untouched():
    n, samples = 3, 100
    a = torch.zeros(n, 256, dtype=torch.uint8, device=DEV)
    b = torch.ones(n, 256, dtype=torch.uint8, device=DEV)
    out = torch.full((n, 256), FILL, dtype=torch.uint8, device=DEV)

    def call(**kw):
        x = dict(a=a.data_ptr(), b=b.data_ptr(), sa=256, sb=256, out=out.data_ptr(), so=256, n=n, samples=samples, bytes=1, num0=1, step=1, den=4)
        x.update(kw)
        raw(x["a"], x["b"], x["sa"], x["sb"], x["out"], x["so"], x["n"], x["samples"], x["bytes"], x["num0"], x["step"], x["den"])

    for bad, text in ((dict(a=None), "payload_mix: null pointer"), (dict(b=None), "payload_mix: null pointer"), (dict(out=None), "payload_mix: null pointer"),
                      (dict(n=0), r"payload_mix: N=0 outside 1\.\.65535"), (dict(n=65536), r"N=65536 outside 1\.\.65535"),
                      (dict(samples=0), "payload_mix: samples=0 must be positive"),
                      (dict(bytes=0), r"payload_mix: sample_bytes 0 not in \{1, 2\}"), (dict(bytes=3), r"sample_bytes 3 not in \{1, 2\}"),
                      (dict(den=1), r"payload_mix: den=1 outside 2\.\.65535"), (dict(den=65536), r"den=65536 outside 2\.\.65535"),
                      (dict(num0=-1), r"payload_mix: k = -1 \+ n \* 1 leaves 0\.\.den=4 within N=3 rows"),
                      (dict(num0=3), r"k = 3 \+ n \* 1 leaves 0\.\.den=4 within N=3 rows"), (dict(num0=1, step=-1), r"k = 1 \+ n \* -1 leaves 0\.\.den=4"),
                      (dict(sa=99), r"payload_mix: strides 99 \(a\), 256 \(b\) neither 0 nor at least the row's 100 bytes"),
                      (dict(sb=-99), r"strides 256 \(a\), -99 \(b\) neither 0 nor at least the row's 100 bytes"),
                      (dict(so=99), r"payload_mix: stride 99 \(out\) shorter than the row's 100 bytes"), (dict(so=0), r"stride 0 \(out\) shorter than"),
                      (dict(bytes=2, a=a.data_ptr() + 1), r"payload_mix: a row of 2-byte samples \(a, b or out\) is not 2-byte aligned"),
                      (dict(bytes=2, out=out.data_ptr() + 1), r"2-byte samples \(a, b or out\) is not 2-byte aligned"),
                      (dict(bytes=2, sb=255), r"payload_mix: strides 256 \(a\), 255 \(b\), 256 \(out\) of 2-byte samples must be even"),
                      (dict(bytes=2, so=-257), r"strides 256 \(a\), 256 \(b\), -257 \(out\) of 2-byte samples must be even"),
                      (dict(out=a.data_ptr()), "payload_mix: out overlaps a or b"), (dict(out=b.data_ptr() + 2 * 256 + 99), "out overlaps a or b"),
                      (dict(out=a.data_ptr() + 99, n=1), "out overlaps a or b")):
        with pytest.raises(RuntimeError, match=text):
            call(**bad)
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == FILL).all(), "a refused call queues nothing"
    call(out=a.data_ptr() + 100, n=1, sa=0, sb=0, so=0)          # N = 1 right behind a's row: no overlap, and a stride names nothing
    call()
    torch.cuda.synchronize()
    host = out.cpu().numpy()
    want = S().payload_mix_host(np.zeros((1, samples), np.uint8), np.ones((1, samples), np.uint8), n, 1, 1, 4, 8)
    assert np.array_equal(host[:, :samples], want) and (host[:, samples:] == FILL).all() and want[:, 0].tolist() == [0, 1, 1]
    assert a.cpu().numpy()[0, 100:200].tolist() == [0] * 100, "0 (den - 1) + 1 + 2 over 4 is 0"
