"""3:2 pulldown removal without a GPU: the definition in numpy (telecine_host, field_diff_host, Cadence, detelecine_host,
detelecine_rate), the refusals of ssm_field_diff_fwd through the library as tests/test_cabi_cpu.py loads it, and the command line's check.

telecine_host cuts a clip out of the endless pulldown of the film; what pulldown removal must give back is read off the same table the
other way round, in film frame numbers (expected_film): the frame at q = 0, 1, 4 is one film frame, the one at q = 2 is dropped, the one at
q = 3 pairs the two fields of one film frame again - and a clip that starts at q = 3 starts with a frame that stays combed."""
import re

import numpy as np
import pytest

from ssm_amd import video as V

H, W, FILM = 8, 6, 17
TAGS = ("420jpeg", "422", "444", "420p10", "422p10", "444p10")


def film_of(tag, n=FILM, seed=0, h=H, w=W):
    layout, bits = V.EXTENDED_TAGS[tag]
    x = np.random.RandomState(seed).randint(0, 256, size=(n, V.frame_bytes(h, w, layout, bits))).astype(np.uint8)
    if bits > 8:
        x.view("<u2")[...] &= (1 << bits) - 1
    return x


def expected_film(n_video, pattern, phase):
    """Per output frame the film frame it is, or ("combed", top, bottom) for a first frame at q = 3; film[0] is the first film frame the
    clip shows a field of."""
    first = min(V.PULLDOWN[pattern][phase])
    out = []
    for m in range(n_video):
        c, q = divmod(phase + m, 5)
        t, b = (4 * c + x - first for x in V.PULLDOWN[pattern][q])
        if q in (0, 1, 4):
            assert t == b
            out.append(t)
        elif q == 3:
            out.append(("combed", t, b) if m == 0 else (t if pattern == 0 else b))          # the film frame whose two fields frames m - 1 and m hold
    return out


@pytest.mark.parametrize("tag", TAGS)
@pytest.mark.parametrize("phase", range(5))
@pytest.mark.parametrize("pattern", (0, 1))
def test_pulldown_and_back_is_the_film_byte_for_byte(pattern, phase, tag):
    layout, bits = V.EXTENDED_TAGS[tag]
    film = film_of(tag, seed=10 * pattern + phase)
    video = V.telecine_host(film, H, W, layout, bits, pattern, phase)
    assert 20 <= len(video) <= 22 and video.shape[1] == film.shape[1]
    got, cadence = V.detelecine_host(video, H, W, layout, bits)
    want = expected_film(len(video), pattern, phase)
    assert len(got) == len(want) and len(want) >= 15
    for i, (out, f) in enumerate(zip(got, want)):
        if isinstance(f, tuple):
            assert phase == 3 and i == 0 and np.array_equal(out, video[0]), "the combed first frame goes out as it stands"
        else:
            assert np.array_equal(out, film[f])
    films = [f for f in want if not isinstance(f, tuple)]
    assert films == list(range(films[0], films[0] + len(films))) and films[0] <= 1, "the film's frames in order, none left out"
    assert cadence.combed_first == (phase == 3)
    # every window finds h = 5 pattern + phi, phi the clip's frame at q = 0, with a clear lock
    h = 5 * pattern + (-phase) % 5
    assert [first for first, _, _, _ in cadence.log] == list(range(1, len(video) - 4, 5))
    for _, got_h, best, second in cadence.log:
        assert got_h == h and best == 0 and second > 0
    assert cadence.dropped == sum(1 for m in range(len(video)) if (phase + m) % 5 == 2)


def test_the_pulldown_table_by_hand():
    """Pattern 0 at phase 0 on four film frames of constant rows: (A, A) (B, B) (B, C) (C, D) (D, D) as (top rows, bottom rows)."""
    film = np.repeat(np.arange(1, 5, dtype=np.uint8)[:, None], V.frame_bytes(4, 2, V.C444), axis=1)
    for pattern, rows in ((0, [(1, 1), (2, 2), (2, 3), (3, 4), (4, 4)]), (1, [(1, 1), (2, 2), (3, 2), (4, 3), (4, 4)])):
        video = V.telecine_host(film, 4, 2, V.C444, 8, pattern, 0)
        assert len(video) == 5
        for frame, (t, b) in zip(video, rows):
            for plane in V.split_planes(frame[None], 4, 2, V.C444):
                assert (plane[0, 0::2] == t).all() and (plane[0, 1::2] == b).all()


def test_field_diff_host_by_hand():
    a = np.zeros((2, 3 * 2 + 5), np.uint8)          # 3 x 2 luma and five bytes that are not looked at
    b = a.copy()
    a[0, :6], b[0, :6] = [1, 2, 30, 40, 5, 6], [0, 0, 0, 0, 0, 9]
    b[1, 6:] = 200
    assert V.field_diff_host(a, b, 3, 2).tolist() == [[1 + 2 + 5 + 3, 70], [0, 0]]
    assert V.field_diff_host(a[:1], b, 3, 2).tolist() == [[11, 70], [1 + 2 + 5 + 6, 70]], "one row against N"
    w = np.zeros((1, 8), np.uint8)
    w.view("<u2")[0] = [65535, 1, 256, 0]
    out = V.field_diff_host(w, np.zeros_like(w), 2, 2, 16)
    assert out.dtype == np.uint64 and out.tolist() == [[65536, 256]]


def test_a_static_clip_ties_everywhere_and_keeps_h_0():
    video = np.repeat(film_of("420jpeg", 1), 16, axis=0)
    got, cadence = V.detelecine_host(video, H, W)
    assert cadence.log == [(1, 0, 0, 0), (6, 0, 0, 0), (11, 0, 0, 0)]
    assert len(got) == 16 - 3 and (got == video[0]).all(), "h = 0 drops frames 2, 7 and 12; a weave of equal frames is the frame"
    assert cadence.dropped == 3


def window(h, low=0, high=9):
    """Five (dT, dB) of a window that starts at a frame n = 1 (mod 5) and fits h exactly: `low` at h's two repeats, `high` elsewhere."""
    out = []
    for n in range(1, 6):
        q, d = V.Cadence.position(n, h), [high, high]
        if q == 2:
            d[h // 5] = low
        if q == 4:
            d[1 - h // 5] = low
        out.append(tuple(d))
    return out


def feed(cadence, sums):
    closed = []
    for dt, db in sums:
        closed += cadence.feed(dt, db)
    return closed


def test_cadence_tie_break_and_carry_over():
    c = V.Cadence()
    assert feed(c, window(7)[:4]) == [] and c.h is None, "nothing is decided before a window is full"
    closed = feed(c, window(7)[4:])
    assert c.h == 7 and [n for n, _ in closed] == [0, 1, 2, 3, 4, 5], "window 0 closes frame 0 with its own five"
    assert c.log == [(1, 7, 0, 9)]
    # an all-equal window ties all ten: the previous hypothesis is among them and wins
    assert [n for n, _ in feed(c, [(4, 4)] * 5)] == [6, 7, 8, 9, 10] and c.h == 7 and c.log[-1] == (6, 7, 8, 8)
    # h = 3 and h = 8 tie at the minimum, 7 is not among them: the lowest wins
    both = [tuple(min(a, b) for a, b in zip(x, y)) for x, y in zip(window(3), window(8))]
    feed(c, both)
    assert c.h == 3 and c.log[-1] == (11, 3, 0, 0)
    # the same tie again: now 3 is the previous one; then 8 alone
    feed(c, both)
    assert c.h == 3
    feed(c, window(8, low=1))
    assert c.h == 8 and c.log[-1] == (21, 8, 2, 10)
    # on a fresh Cadence the first window's tie goes to the lowest h
    d = V.Cadence()
    feed(d, both)
    assert d.h == 3


def test_cadence_actions():
    c = V.Cadence()
    acts = dict(feed(c, window(0)))          # pattern 0, frame 0 at q = 0
    assert acts == {0: (0, 0), 1: (1, 1), 2: None, 3: (3, 2), 4: (4, 4), 5: (5, 5)} and not c.combed_first
    c = V.Cadence()
    acts = dict(feed(c, window(5 + 2)))      # pattern 1, phi = 2: frame 0 at q = 3, frame 4 at q = 2, frame 5 at q = 3
    assert acts == {0: (0, 0), 1: (1, 1), 2: (2, 2), 3: (3, 3), 4: None, 5: (4, 5)} and c.combed_first and c.dropped == 1


def test_a_short_tail_keeps_the_last_hypothesis():
    c = V.Cadence()
    feed(c, window(1))
    assert feed(c, [(5, 5)] * 3) == []
    tail = c.end()
    # h = 1: q = (n - 1) % 5, frames 6, 7, 8 sit at q = 0, 1, 2
    assert tail == [(6, (6, 6)), (7, (7, 7)), (8, None)] and c.h == 1 and len(c.log) == 1
    layout, bits = V.EXTENDED_TAGS["420jpeg"]
    film = film_of("420jpeg", 8)
    video = V.telecine_host(film, H, W, layout, bits, 0, 0)[:9]          # one window, then the tail B, (B, C), (C, D)
    got, cadence = V.detelecine_host(video, H, W, layout, bits)
    assert len(cadence.log) == 1 and np.array_equal(got, film[:7]), "A B C D of the first cycle, then A, B and the tail's weave C"


@pytest.mark.parametrize("n", range(1, 6))
def test_clips_under_six_frames_are_refused(n):
    with pytest.raises(V.Y4MError, match="the clip has %d frames, fewer than 6" % n):
        V.detelecine_host(film_of("420jpeg", n), H, W)
    c = V.Cadence()
    feed(c, [(0, 0)] * (n - 1))
    with pytest.raises(V.Y4MError, match="fewer than 6"):
        c.end()


def test_heights_without_fields_are_refused():
    with pytest.raises(V.Y4MError, match="a telecined frame has an even number of rows: H=7 is odd"):
        V.detelecine_host(film_of("444", 6, h=7), 7, W, V.C444)
    with pytest.raises(V.Y4MError, match="a telecined frame in 4:2:0 has a multiple of 4 rows, two chroma fields of H/4: H=6 is not"):
        V.detelecine_host(film_of("420jpeg", 6, h=6), 6, W)
    with pytest.raises(V.Y4MError, match="multiple of 4 rows"):
        V.telecine_host(film_of("420jpeg", 6, h=6), 6, W)
    assert len(V.detelecine_host(film_of("422", 6, h=6), 6, W, V.C422)[0]) in (4, 5), "4:2:2 and 4:4:4 only need an even H"


def test_output_rate():
    assert V.detelecine_rate((30000, 1001)) == (24000, 1001)
    assert V.detelecine_rate((30, 1)) == (24, 1)
    assert V.detelecine_rate((60000, 1001)) == (48000, 1001) and V.detelecine_rate((25, 1)) == (20, 1)


# ---- ssm_field_diff_fwd: every refusal, nothing queued --------------------------------------------------------------------------------
P, Q, SUMS = 0x10000, 0x20000, 0x30000          # addresses that are never followed: every call below is refused before anything is queued


@pytest.mark.parametrize("args,message", [
    ((None, Q, 64, 64, 1, 8, 8, 1, SUMS), "field_diff: null pointer"),
    ((P, None, 64, 64, 1, 8, 8, 1, SUMS), "field_diff: null pointer"),
    ((P, Q, 64, 64, 1, 8, 8, 1, None), "field_diff: null pointer"),
    ((P, Q, 64, 64, 0, 8, 8, 1, SUMS), "field_diff: N=0 outside 1..65535"),
    ((P, Q, 64, 64, 65536, 8, 8, 1, SUMS), "field_diff: N=65536 outside 1..65535"),
    ((P, Q, 64, 64, 1, 0, 8, 1, SUMS), "field_diff: bad plane size 0x8"),
    ((P, Q, 64, 64, 1, 8, -1, 1, SUMS), "field_diff: bad plane size 8x-1"),
    ((P, Q, 64, 64, 1, 8, 8, 0, SUMS), "field_diff: sample_bytes 0 not in {1, 2}"),
    ((P, Q, 64, 64, 1, 8, 8, 3, SUMS), "field_diff: sample_bytes 3 not in {1, 2}"),
    ((P, Q, 63, 64, 2, 8, 8, 1, SUMS), "field_diff: strides 63 (a), 64 (b) neither 0 nor at least the plane's 64 bytes"),
    ((P, Q, 64, -63, 2, 8, 8, 1, SUMS), "field_diff: strides 64 (a), -63 (b) neither 0 nor at least the plane's 64 bytes"),
    ((P, Q, 0, 127, 1, 8, 8, 2, SUMS), "field_diff: strides 0 (a), 127 (b) neither 0 nor at least the plane's 128 bytes"),
    ((P + 1, Q, 128, 128, 2, 8, 8, 2, SUMS), "field_diff: a payload of 2-byte samples (a or b) is not 2-byte aligned"),
    ((P, Q + 1, 128, 128, 2, 8, 8, 2, SUMS), "field_diff: a payload of 2-byte samples (a or b) is not 2-byte aligned"),
    ((P, Q, 129, 128, 2, 8, 8, 2, SUMS), "field_diff: strides 129 (a), 128 (b) of 2-byte samples must be even"),
    ((P, Q, 64, 64, 2, 8, 8, 1, SUMS + 4), "field_diff: sums is not 8-byte aligned"),
    ((P, Q, 0, 0, 1, 2147483647, 17, 1, SUMS), "field_diff: a plane of 36507221999 bytes is more than the grid takes"),
])
def test_field_diff_refusals(args, message):
    from ssm_amd import hipbind as hb
    lib = hb.load()
    assert lib.ssm_field_diff_fwd(*args, None) == -1
    assert lib.ssm_last_error_string().decode() == message


def test_field_diff_refusals_come_in_the_documented_order():
    """A call that is wrong in every way names the first of: pointers, N, H and W, sample_bytes, strides, 2-byte alignment, sums, the grid."""
    from ssm_amd import hipbind as hb
    lib = hb.load()
    err = lambda: lib.ssm_last_error_string().decode()  # noqa: E731
    huge = (2147483647, 17)
    assert lib.ssm_field_diff_fwd(None, Q + 1, 3, 3, 0, 0, 0, 5, SUMS + 4, None) == -1 and "null pointer" in err()
    assert lib.ssm_field_diff_fwd(P + 1, Q + 1, 3, 3, 0, 0, 0, 5, SUMS + 4, None) == -1 and "N=0" in err()
    assert lib.ssm_field_diff_fwd(P + 1, Q + 1, 3, 3, 2, 0, 0, 5, SUMS + 4, None) == -1 and "bad plane size" in err()
    assert lib.ssm_field_diff_fwd(P + 1, Q + 1, 3, 3, 2, *huge, 5, SUMS + 4, None) == -1 and "sample_bytes 5" in err()
    assert lib.ssm_field_diff_fwd(P + 1, Q + 1, 3, 3, 2, *huge, 2, SUMS + 4, None) == -1 and "neither 0 nor at least" in err()
    assert lib.ssm_field_diff_fwd(P + 1, Q + 1, 0, 1 << 40 | 1, 2, *huge, 2, SUMS + 4, None) == -1 and "not 2-byte aligned" in err()
    assert lib.ssm_field_diff_fwd(P, Q, 0, 1 << 40 | 1, 2, *huge, 2, SUMS + 4, None) == -1 and "must be even" in err()
    assert lib.ssm_field_diff_fwd(P, Q, 0, 1 << 40, 2, *huge, 2, SUMS + 4, None) == -1 and "sums is not 8-byte aligned" in err()
    assert lib.ssm_field_diff_fwd(P, Q, 0, 1 << 40, 2, *huge, 2, SUMS, None) == -1 and "more than the grid takes" in err()


# ---- command line -----------------------------------------------------------------------------------------------------------------------
BASE = ["-c", "x.ini", "--expt", "e", "--log", "l", "--input", "-", "--output", "-"]


def test_cli_flag_goes_with_everything_else():
    import interpolate_video as cli
    a = cli.getargs(BASE)
    assert a.detelecine is False and a.upsample_rate == 8, "without the flag the tool is as it was"
    a = cli.getargs(BASE + ["--detelecine"])
    assert a.detelecine and a.upsample_rate == 8 and a.deinterlace is None
    a = cli.getargs(BASE + ["--detelecine", "--fps", "60000:1001", "--shutter", "180", "--tile", "64x64"])
    assert a.detelecine and a.fps == (60000, 1001) and a.tile == (64, 64)
    assert cli.getargs(BASE + ["--detelecine", "--upsample_rate", "2", "--scene_cut", "0.1", "--slowmo"]).scene_cut is not None


def test_cli_refuses_detelecine_with_deinterlace(capsys):
    import interpolate_video as cli
    with pytest.raises(SystemExit) as e:
        cli.getargs(BASE + ["--detelecine", "--deinterlace", "auto"])
    assert e.value.code == 2
    assert re.search(r"--detelecine does not go together with --deinterlace", capsys.readouterr().err)
