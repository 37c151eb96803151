"""The field order from the data without a GPU: the definition in numpy (field_order_sums_host against a literal triple loop),
the kind of a frame at both ratios, the verdict's majorities, the classification of the texture clips of tests/field_clips.py, the parsers,
the refusals of ssm_field_order_sums_fwd through the library as tests/test_cabi_cpu.py loads it, and the command line's checks."""
import os
import re
import sys

import numpy as np
import pytest

from ssm_amd import video as V

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import field_clips as FC  # noqa: E402


def by_loops(p, c, n, h, w):
    """(A0, A1, D) of three planes [h][w] of Python integers, as the header writes the definition."""
    a0 = a1 = d = 0
    for y in range(1, h - 1):
        ep = en = ec = 0
        for x in range(w):
            s = c[y - 1][x] + c[y + 1][x]
            ep += abs(s - 2 * p[y][x])
            en += abs(s - 2 * n[y][x])
            ec += abs(s - 2 * c[y][x])
        if y % 2 == 0:
            a0, a1 = a0 + ep, a1 + en
        else:
            a0, a1 = a0 + en, a1 + ep
        d += ec
    return [a0, a1, d]


@pytest.mark.parametrize("bits", (8, 16))
@pytest.mark.parametrize("h,w", ((1, 4), (2, 3), (3, 1), (3, 5), (4, 2), (5, 3), (6, 7)))
def test_sums_host_equals_the_triple_loop(h, w, bits):
    rng = np.random.RandomState(100 * h + w + bits)
    sb = V.sample_bytes(bits)
    planes = rng.randint(0, 256, size=(3, 2, h * w * sb + 3)).astype(np.uint8)          # three bytes behind every plane are not looked at
    got = V.field_order_sums_host(planes[0], planes[1], planes[2], h, w, bits)
    assert got.dtype == np.uint64 and got.shape == (2, 3)

    def plane(x, i):
        return x[i, :h * w * sb].copy().view("<u2" if sb == 2 else np.uint8).reshape(h, w).tolist()

    for i in range(2):
        assert got[i].tolist() == by_loops(plane(planes[0], i), plane(planes[1], i), plane(planes[2], i), h, w), (h, w, bits, i)
    if h < 3:
        assert not got.any(), "no row has a row above and a row below"
    one = V.field_order_sums_host(planes[0][:1], planes[1], planes[2], h, w, bits)
    assert one[1].tolist() == by_loops(plane(planes[0], 0), plane(planes[1], 1), plane(planes[2], 1), h, w), "a single row goes against every one"


def test_sums_host_by_hand():
    """3 x 2: one inner row, y = 1, odd: A0 takes E_n, A1 takes E_p.  c rows (1, 2), (9, 9), (5, 8): s = (6, 10)."""
    c = np.array([[1, 2, 9, 9, 5, 8]], np.uint8)
    p = np.array([[0, 0, 3, 4, 0, 0]], np.uint8)          # 2 p = (6, 8): E_p = 0 + 2
    n = np.array([[0, 0, 0, 9, 0, 0]], np.uint8)          # 2 n = (0, 18): E_n = 6 + 8
    assert V.field_order_sums_host(p, c, n, 3, 2).tolist() == [[14, 2, 12 + 8]]
    w = np.array([[0, 65535, 0]], "<u2").view(np.uint8)          # 3 x 1 words: s = 0 against 2 * 65535
    assert V.field_order_sums_host(w, w, w, 3, 1, 16).tolist() == [[131070, 131070, 131070]]


def test_kind_at_and_beside_both_ratios():
    assert V.field_kind(26, 25, 0) == "P", "25 A0 = 26 A1 is not above the ratio"
    assert V.field_kind(27, 25, 0) == "T" and V.field_kind(2601, 2500, 10 ** 9) == "T"
    assert V.field_kind(25, 26, 0) == "P" and V.field_kind(25, 27, 0) == "B" and V.field_kind(2500, 2601, 10 ** 9) == "B"
    assert V.field_kind(2599, 2500, 0) == "P"
    # 2 min > 3 D
    assert V.field_kind(30, 31, 20) == "U", "2 * 30 = 3 * 20 is not above the ratio"
    assert V.field_kind(31, 30, 20) == "U" and V.field_kind(31, 31, 20) == "P" and V.field_kind(30, 30, 19) == "P"
    assert V.field_kind(5, 5, 5) == "U", "a still: A0 = A1 = D"
    assert V.field_kind(0, 0, 0) == "U"
    assert V.field_kind(np.uint64(2 ** 63), np.uint64(2 ** 62), np.uint64(0)) == "T", "Python integers, no overflow"


def test_verdict_majorities_ties_and_short_probes():
    v = V.FieldVerdict("TTTB")
    assert (v.kinds, v.counts, v.verdict) == ("TTTB", (3, 1, 0, 0), "tff")
    assert "3 top field first, 1 bottom field first, 0 progressive, 0 undetermined" in v.note and v.note.endswith(": tff")
    assert V.FieldVerdict("BBPU").verdict == "bff", "U is not in the denominator: 2 of 3"
    assert V.FieldVerdict("PPPTB").verdict == "progressive"
    assert V.FieldVerdict("TB").verdict is None and V.FieldVerdict("TTBB").verdict is None, "a tie is no majority"
    assert V.FieldVerdict("TBP").verdict is None and V.FieldVerdict("TTBP").verdict is None, "2 * 2 = 4 is not above 4"
    assert V.FieldVerdict("TUUUUU").verdict == "tff" and V.FieldVerdict("UUUU").verdict is None
    empty = V.FieldVerdict("")
    assert empty.verdict is None and empty.counts == (0, 0, 0, 0) and "no verdict" in empty.note
    # fewer than 3 probed frames have no inner frame
    for m in (0, 1, 2):
        assert V.FieldVerdict.of_sums(np.zeros((max(m - 2, 0), 3), np.uint64)).verdict is None
    assert V.FieldVerdict.of_sums(np.array([[27, 25, 0], [27, 25, 3]], np.uint64)).kinds == "TT"


@pytest.mark.parametrize("v", (1.0, 0.25))
@pytest.mark.parametrize("h,w", ((16, 24), (36, 52), (37, 53)))
def test_every_inner_frame_of_the_texture_clips_is_of_its_kind(h, w, v):
    for kind, letter, verdict in (("tff", "T", "tff"), ("bff", "B", "bff"), ("progressive", "P", "progressive"), ("still", "U", None)):
        luma = FC.luma_clip(kind, 10, h, w, v).reshape(10, -1)
        sums = V.field_order_sums_host(luma[:-2], luma[1:-1], luma[2:], h, w)
        got = V.FieldVerdict.of_sums(sums)
        assert got.kinds == letter * 8, (kind, h, w, v, sums.tolist())
        assert got.verdict == verdict
        if kind == "still":
            assert all(a0 == a1 == d for a0, a1, d in sums.tolist())


def test_ten_bit_words_classify_as_the_bytes_do():
    pay = FC.payloads("bff", 6, 16, 24, "422p10")
    sums = V.field_order_sums_host(pay[:-2], pay[1:-1], pay[2:], 16, 24, 10)
    luma = FC.luma_clip("bff", 6, 16, 24).reshape(6, -1)
    assert (sums == 4 * V.field_order_sums_host(luma[:-2], luma[1:-1], luma[2:], 16, 24)).all()
    assert V.FieldVerdict.of_sums(sums).verdict == "bff"


# ---- the parsers ------------------------------------------------------------------------------------------------------------------------
def test_parse_field_probe():
    assert V.parse_field_probe(3) == 3 and V.parse_field_probe(" 48 ") == 48 and V.FIELD_PROBE == 48
    for bad in (0, -1, "0", "x", "1.5", 2.5, True, None):
        with pytest.raises(ValueError, match=r"field_probe, the frames the field order is decided on, is a whole number of at least 1 \(got"):
            V.parse_field_probe(bad)


def test_deinterlace_parser_and_header_rule_are_as_they_were():
    assert V.DEINTERLACE == ("auto", "tff", "bff")
    with pytest.raises(ValueError, match="this one says Ip"):
        V.field_order("auto", "p")


class _Recurrent:
    recurrent = True


def test_interpolator_refuses_a_bad_probe_and_a_recurrent_model():
    import configparser
    cfg = configparser.RawConfigParser()
    cfg.read_dict({"TRAIN": {"N_FRAMES": "2"}})
    with pytest.raises(ValueError, match="field_probe, the frames"):
        V.VideoInterpolator(object(), cfg, field_probe=0)
    with pytest.raises(ValueError, match="field_probe together with a recurrent model is not available"):
        V.VideoInterpolator(_Recurrent(), cfg, field_probe=True)
    vi = V.VideoInterpolator(object(), cfg)
    assert vi.field_probe_option is None and vi.field_probe is None
    assert V.VideoInterpolator(object(), cfg, field_probe=True).field_probe_option == 48
    assert V.VideoInterpolator(object(), cfg, field_probe=5, deinterlace="auto").field_probe_option == 5


# ---- ssm_field_order_sums_fwd: every refusal, nothing queued ----------------------------------------------------------------------------
P, C, N, SUMS = 0x10000, 0x20000, 0x30000, 0x40000          # addresses that are never followed: every call below is refused first


@pytest.mark.parametrize("args,message", [
    ((None, C, N, 64, 64, 64, 1, 8, 8, 1, SUMS), "field_order_sums: null pointer"),
    ((P, None, N, 64, 64, 64, 1, 8, 8, 1, SUMS), "field_order_sums: null pointer"),
    ((P, C, None, 64, 64, 64, 1, 8, 8, 1, SUMS), "field_order_sums: null pointer"),
    ((P, C, N, 64, 64, 64, 1, 8, 8, 1, None), "field_order_sums: null pointer"),
    ((P, C, N, 64, 64, 64, 0, 8, 8, 1, SUMS), "field_order_sums: N=0 outside 1..65535"),
    ((P, C, N, 64, 64, 64, 65536, 8, 8, 1, SUMS), "field_order_sums: N=65536 outside 1..65535"),
    ((P, C, N, 64, 64, 64, 1, 0, 8, 1, SUMS), "field_order_sums: bad plane size 0x8"),
    ((P, C, N, 64, 64, 64, 1, 8, -1, 1, SUMS), "field_order_sums: bad plane size 8x-1"),
    ((P, C, N, 64, 64, 64, 1, 8, 8, 0, SUMS), "field_order_sums: sample_bytes 0 not in {1, 2}"),
    ((P, C, N, 64, 64, 64, 1, 8, 8, 3, SUMS), "field_order_sums: sample_bytes 3 not in {1, 2}"),
    ((P, C, N, 63, 64, 64, 2, 8, 8, 1, SUMS), "field_order_sums: strides 63 (p), 64 (c), 64 (n) neither 0 nor at least the plane's 64 bytes"),
    ((P, C, N, 64, -63, 0, 2, 8, 8, 1, SUMS), "field_order_sums: strides 64 (p), -63 (c), 0 (n) neither 0 nor at least the plane's 64 bytes"),
    ((P, C, N, 0, -128, 127, 1, 8, 8, 2, SUMS), "field_order_sums: strides 0 (p), -128 (c), 127 (n) neither 0 nor at least the plane's 128 bytes"),
    ((P + 1, C, N, 128, 128, 128, 2, 8, 8, 2, SUMS), "field_order_sums: a payload of 2-byte samples (p, c or n) is not 2-byte aligned"),
    ((P, C + 1, N, 128, 128, 128, 2, 8, 8, 2, SUMS), "field_order_sums: a payload of 2-byte samples (p, c or n) is not 2-byte aligned"),
    ((P, C, N + 1, 128, 128, 128, 2, 8, 8, 2, SUMS), "field_order_sums: a payload of 2-byte samples (p, c or n) is not 2-byte aligned"),
    ((P, C, N, 128, 128, 129, 2, 8, 8, 2, SUMS), "field_order_sums: strides 128 (p), 128 (c), 129 (n) of 2-byte samples must be even"),
    ((P, C, N, 64, 64, 64, 2, 8, 8, 1, SUMS + 4), "field_order_sums: sums is not 8-byte aligned"),
    ((P, C, N, 0, 0, 0, 1, 2147483647, 17, 1, SUMS), "field_order_sums: a plane of 36507221999 bytes is more than the grid takes"),
])
def test_field_order_sums_refusals(args, message):
    from ssm_amd import hipbind as hb
    lib = hb.load()
    assert lib.ssm_field_order_sums_fwd(*args, None) == -1
    assert lib.ssm_last_error_string().decode() == message


def test_field_order_sums_refusals_come_in_the_documented_order():
    """A call that is wrong in every way names the first of: pointers, N, H and W, sample_bytes, strides, 2-byte alignment, sums, the grid."""
    from ssm_amd import hipbind as hb
    lib = hb.load()
    f = lib.ssm_field_order_sums_fwd
    err = lambda: lib.ssm_last_error_string().decode()  # noqa: E731
    huge = (2147483647, 17)
    assert f(None, C + 1, N, 3, 3, 3, 0, 0, 0, 5, SUMS + 4, None) == -1 and "null pointer" in err()
    assert f(P + 1, C + 1, N, 3, 3, 3, 0, 0, 0, 5, SUMS + 4, None) == -1 and "N=0" in err()
    assert f(P + 1, C + 1, N, 3, 3, 3, 2, 0, 0, 5, SUMS + 4, None) == -1 and "bad plane size" in err()
    assert f(P + 1, C + 1, N, 3, 3, 3, 2, *huge, 5, SUMS + 4, None) == -1 and "sample_bytes 5" in err()
    assert f(P + 1, C + 1, N, 3, 3, 3, 2, *huge, 2, SUMS + 4, None) == -1 and "neither 0 nor at least" in err()
    assert f(P + 1, C + 1, N, 0, 0, 1 << 40 | 1, 2, *huge, 2, SUMS + 4, None) == -1 and "not 2-byte aligned" in err()
    assert f(P, C, N, 0, 0, 1 << 40 | 1, 2, *huge, 2, SUMS + 4, None) == -1 and "must be even" in err()
    assert f(P, C, N, 0, 0, 1 << 40, 2, *huge, 2, SUMS + 4, None) == -1 and "sums is not 8-byte aligned" in err()
    assert f(P, C, N, 0, 0, 1 << 40, 2, *huge, 2, SUMS, None) == -1 and "more than the grid takes" in err()


# ---- command line -----------------------------------------------------------------------------------------------------------------------
BASE = ["-c", "x.ini", "--expt", "e", "--log", "l", "--input", "-", "--output", "-"]


def test_cli_flag_is_off_by_default_and_takes_an_optional_count():
    import interpolate_video as cli
    assert cli.getargs(BASE).field_probe is None, "without the flag the tool is as it was"
    assert cli.getargs(BASE + ["--field_probe"]).field_probe == 48
    a = cli.getargs(BASE + ["--deinterlace", "auto", "--field_probe", "12"])
    assert a.field_probe == 12 and a.deinterlace == "auto"
    assert cli.getargs(BASE + ["--field_probe", "--deinterlace", "bff"]).deinterlace == "bff"
    assert cli.getargs(BASE + ["--field_probe", "--fps", "60", "--active", "auto"]).field_probe == 48, "a report goes with every mode"


def test_cli_refuses_a_bad_count_and_detelecine(capsys):
    import interpolate_video as cli
    with pytest.raises(SystemExit) as e:
        cli.getargs(BASE + ["--field_probe", "0"])
    assert e.value.code == 2 and re.search(r"field_probe, the frames the field order is decided on", capsys.readouterr().err)
    with pytest.raises(SystemExit) as e:
        cli.getargs(BASE + ["--field_probe", "--detelecine"])
    assert e.value.code == 2
    assert re.search(r"--field_probe does not go together with --detelecine: a telecined clip is a mixture", capsys.readouterr().err)
