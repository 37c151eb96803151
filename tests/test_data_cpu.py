"""No-GPU checks of ssm_amd.data: the clip lists, the index plans, the epoch's draws and shards, the frame sources, scripts/utils/
pack_clips.py, and the numpy float32 yardstick (augment_host) that the kernel of csrc/ssm_data.hip is held to bit for bit in
tests/test_hip_data.py.  The yardstick itself is held here to an independent float64 evaluation of the definition in include/ssm_hip.h.

Bars of the float64 comparison, u = 2^-24, in normalised units.
  Integer mode.  The 8-bit value s is exact.  q = s / 255 rounds once: u |q| <= u.  fl(mean) is off by <= u |mean| < u, the difference
  rounds once more at u |d| < u: 3u absolute on d, 3u / 0.224 = 13.4u after the division by std >= 0.224.  fl(std) and the quotient
  round at u each, relative, of |n| <= 2.7: 5.4u.  Sum 18.8u; the bar is 20u = 1.2e-6 (test_video_cpu.py derives 1e-5 for the same
  expression behind a colour conversion; this one starts from exact values).
  Affine mode.  The float64 evaluation uses the same fp32 coefficients, so only the evaluation differs.  fp32 u = (a0 x + a1 y) + a2
  carries one rounding per product and per sum, each <= u times the magnitude M = |a0| (tw - 1) + |a1| (th - 1) + |a2| of what it
  rounds: du <= 4u M (two products, two sums); likewise dv.  The bilinear sample is continuous in (u, v), also across integer
  coordinates (the weight of the tap that changes is 0 there: a differing floor costs no jump) and across the border (taps outside are
  0), and moves by at most 255 per pixel of displacement in each axis, so |ds| <= 255 (du + dv).  Its own arithmetic - two subtractions
  for the weights, then three levels of product + sum on values <= 255 - adds <= 12u 255.  In normalised units: ds / 255 / 0.224, plus
  the integer-mode bar for the normalise expression."""
import configparser
import os
import subprocess
import sys

import numpy as np
import pytest

from ssm_amd import data as D
from ssm_amd.config import CONFIG_DIR
from ssm_amd.weights import IMAGENET_MEAN, IMAGENET_STD

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -24
BAR_INT = 20 * U


def make_cfg(tmp_path, dataset="ADOBE", batch=2, crop=(32, 48), n_frames=2, size=(96, 128), t_sample="RANDOM"):
    cfg = configparser.RawConfigParser()
    cfg.read(os.path.join(CONFIG_DIR, "superslomo_original.ini"))
    cfg.set("DATA", "DATASET", dataset)
    for sec in ("ADOBE_DATA", "NFS_DATA", "VIMEO_DATA"):
        cfg.set(sec, "TRAINPATHS", str(tmp_path / (sec.lower() + "_train.txt")))
        cfg.set(sec, "H_IN", str(size[0]))
        cfg.set(sec, "W_IN", str(size[1]))
    cfg.set("VIMEO_DATA", "ROOTDIR", str(tmp_path / "vimeo"))
    cfg.set("TRAIN", "BATCH_SIZE", str(batch))
    cfg.set("TRAIN", "CROP_IMH", str(crop[0]))
    cfg.set("TRAIN", "CROP_IMW", str(crop[1]))
    cfg.set("TRAIN", "N_FRAMES", str(n_frames))
    cfg.set("DATALOADER", "T_SAMPLE", t_sample)
    return cfg


def frames_rgb(n, h, w, seed):
    """[n, h, w, 3] uint8: a smooth moving pattern plus noise (every byte value occurs)."""
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    base = np.stack([(3 * xx + 5 * yy) % 256, (7 * xx + 2 * yy + 40) % 256, (xx * yy + 11) % 256], -1)
    return np.stack([((base + 9 * i + rng.randint(0, 24, base.shape)) % 256).astype(np.uint8) for i in range(n)])


def write_png_clips(tmp_path, n_clips, n_frames, h, w, name="adobe_data_train.txt", leading_count=True, seed=0):
    """PNG clips in the ADOBE list format; returns ([frames [T,h,w,3]], list path)."""
    from PIL import Image
    clips, lines = [], ["%d" % n_clips] if leading_count else []
    for c in range(n_clips):
        fr = frames_rgb(n_frames, h, w, seed + c)
        d = tmp_path / ("clip_%s_%03d" % (name.split("_")[0], c))
        d.mkdir(parents=True, exist_ok=True)
        lines.append("%d" % n_frames)
        for k in range(n_frames):
            Image.fromarray(fr[k]).save(str(d / ("%04d.png" % k)))
            lines.append(str(d / ("%04d.png" % k)))
        clips.append(fr)
    (tmp_path / name).write_text("\n".join(lines) + "\n")
    return clips, tmp_path / name


# ---- clip lists --------------------------------------------------------------------------------------------------------------------
def test_counted_list_with_a_three_digit_count_and_a_leading_total():
    a, b = ["a/%04d.png" % i for i in range(120)], ["b/%d.png" % i for i in range(9)]
    lines = ["2", "120"] + a + ["9"] + b
    assert D.parse_counted_list([ln + "\n" for ln in lines]) == [a, b]
    assert D.parse_counted_list(lines[1:]) == [a, b]          # no leading total
    with pytest.raises(ValueError, match="announces 9 frames"):
        D.parse_counted_list(["9"] + b[:5])


def test_vimeo_and_all_lists(tmp_path):
    cfg = make_cfg(tmp_path, "ALL")
    (tmp_path / "adobe_data_train.txt").write_text("2\n100\n" + "".join("a/%d.png\n" % i for i in range(100)) + "9\n" + "".join("b/%d.png\n" % i for i in range(9)))
    (tmp_path / "nfs_data_train.txt").write_text("9\n" + "".join("n/%d.jpg\n" % i for i in range(9)))
    (tmp_path / "vimeo_data_train.txt").write_text("00001/0001\n00002/0007\n")
    vim = D.read_clip_list(cfg, "TRAIN", "VIMEO")
    root = str(tmp_path / "vimeo")
    assert vim == [("vimeo", ["%s/sequences/%s/im%d.png" % (root, s, i) for i in range(1, 8)]) for s in ("00001/0001", "00002/0007")]
    allc = D.read_clip_list(cfg, "TRAIN")
    assert [k for k, _ in allc] == ["window"] * 3 + ["vimeo"] * 2
    assert [len(p) for _, p in allc] == [100, 9, 9, 7, 7] and allc[0][1][0] == "a/0.png" and allc[2][1][0] == "n/0.jpg" and allc[3:] == vim
    cfg.set("DATA", "DATASET", "SLOWFLOW")
    with pytest.raises(ValueError, match="no training reader"):
        D.read_clip_list(cfg, "TRAIN")


# ---- index plans -------------------------------------------------------------------------------------------------------------------
def test_index_plans_literal_values():
    assert D.window_plan(2, 3) == ([0, 8], [3], 0.375)
    for s in range(1, 8):
        assert D.window_plan(4, s) == ([0, 8, 16, 24], [s, 8 + s, 16 + s], s / 8.0)
    assert D.window_plan(8, 7)[0][-1] == 56 == D.reqd_images(8) - 1 and [D.reqd_images(n) for n in (2, 4, 6, 8)] == [9, 25, 41, 57]
    assert D.vimeo_plan(2, 1) == ([0, 2], [1], 0.5) and D.vimeo_plan(2, 3) == ([2, 4], [3], 0.5) and D.vimeo_plan(2, 5) == ([4, 6], [5], 0.5)
    assert D.vimeo_plan(4, 1) == ([0, 0, 2, 4], [0, 1, 3], 0.5)
    assert D.vimeo_plan(4, 3) == ([0, 2, 4, 6], [1, 3, 5], 0.5)
    assert D.vimeo_plan(4, 5) == ([2, 4, 6, 6], [3, 5, 6], 0.5)
    with pytest.raises(ValueError):
        D.vimeo_plan(6, 3)
    assert D.sample_s("MIDDLE", 0.9) == 4
    assert sorted({D.sample_s("RANDOM", u) for u in np.linspace(0, 1, 141, endpoint=False)}) == list(range(1, 8))
    with pytest.raises(NotImplementedError):
        D.sample_s("NIL", 0.5)


def test_sample_plan_reads_the_window_reversal_and_t(tmp_path):
    paths = ["f%03d" % i for i in range(30)]
    u = np.array([0.5, 0.0, 2.5 / 7, 0.0, 0.999999, 0.9, 0.0, 0.0, 0.5])
    sp = D.plan_sample(0, "window", paths, u, 2, "RANDOM", 32, 48)
    start = 11                                          # floor(0.5 * (30 - 9 + 1))
    assert sp.paths == [paths[start], paths[start + 8], paths[start + 3]] and sp.t == 0.375 and not sp.hflip and sp.affine is None
    u[1] = 0.75                                         # reversed in time: the window runs backwards
    sp = D.plan_sample(0, "window", paths, u, 2, "RANDOM", 32, 48, flip=True, rotate=True)
    assert sp.paths == [paths[start + 8], paths[start], paths[start + 5]] and sp.hflip and sp.affine.dtype == np.float32
    r = sp.record(96, 128, 32, 48)
    assert (int(r["y1"]), int(r["x1"])) == (0, 80) and int(r["flags"]) == D.HFLIP | D.AFFINE
    sp = D.plan_sample(0, "vimeo", ["im%d" % i for i in range(1, 8)], u, 2, "NIL", 32, 48)          # septuplets ignore T_SAMPLE: t = 0.5
    assert sp.t == 0.5 and len(sp.paths) == 3
    with pytest.raises(D.ClipReadError, match="f000"):
        D.plan_sample(0, "window", paths[:8], u, 2, "RANDOM", 32, 48)
    cfg = make_cfg(tmp_path, t_sample="NIL")
    (tmp_path / "adobe_data_train.txt").write_text("9\n" + "".join("a/%d.png\n" % i for i in range(9)))
    with pytest.raises(NotImplementedError):
        D.ClipLoader(cfg, "TRAIN", None)


# ---- draws and shards --------------------------------------------------------------------------------------------------------------
def test_records_do_not_depend_on_the_worker_count_and_epochs_differ(tmp_path):
    write_png_clips(tmp_path, 6, 12, 96, 128)
    cfg = make_cfg(tmp_path)
    runs = {}
    for nw, epoch in ((1, 0), (4, 0), (4, 1)):
        ld = D.ClipLoader(cfg, "TRAIN", None, 0, 1, seed=5, n_workers=nw, flip=True, rotate=True)
        assert ld.n_workers == min(nw, len(os.sched_getaffinity(0)), 16)
        runs[nw, epoch] = [(tab.tobytes(), [f.tobytes() for f in fr], t.tobytes(), [sp.index for sp in plans])
                           for plans, tab, fr, t in ld.host_batches(epoch)]
    assert len(runs[1, 0]) == 3 and runs[1, 0] == runs[4, 0]
    assert runs[4, 0] != runs[4, 1] and [b[3] for b in runs[4, 0]] != [b[3] for b in runs[4, 1]]
    assert D.worker_count(cfg, 64) <= 16 and D.worker_count(cfg) == min(12, len(os.sched_getaffinity(0)), 16)


@pytest.mark.parametrize("world", [2, 8])
def test_shards_are_disjoint_equal_and_cover_the_permutation(tmp_path, world):
    cfg = make_cfg(tmp_path, batch=3)
    (tmp_path / "adobe_data_train.txt").write_text("".join("9\n" + "".join("c%d/%d.png\n" % (c, i) for i in range(9)) for c in range(100)))
    per_rank = []
    for rank in range(world):
        ld = D.ClipLoader(cfg, "TRAIN", None, rank, world, seed=3)
        batches = ld.plan_epoch(2)
        assert len(batches) == len(ld) == 100 // (3 * world) and all(len(b) == 3 for b in batches)
        per_rank.append([sp.index for b in batches for sp in b])
    perm = D.epoch_rng(3, 2).permutation(100)
    kept = len(per_rank[0]) * world
    flat = [i for r in per_rank for i in r]
    assert len(set(flat)) == len(flat) == kept and set(flat) == set(int(i) for i in perm[:kept])
    for rank in range(world):
        assert per_rank[rank] == [int(i) for i in perm[rank:kept:world]]


def test_crop_origins_reach_both_ends_and_a_fitting_side_works():
    h, w, th, tw = 40, 56, 32, 48
    rng = D.epoch_rng(1, 0)
    seen_x, seen_y = set(), set()
    for _ in range(400):
        u = rng.random(D.N_DRAWS)
        r = D.plan_sample(0, "vimeo", list("abcdefg"), u, 2, "RANDOM", th, tw).record(h, w, th, tw)
        seen_y.add(int(r["y1"]))
        seen_x.add(int(r["x1"]))
    assert seen_x == set(range(w - tw + 1)) and seen_y == set(range(h - th + 1))
    sp = D.plan_sample(0, "vimeo", list("abcdefg"), np.full(D.N_DRAWS, 0.999), 2, "RANDOM", th, tw)
    r = sp.record(40, 48, th, tw)                       # w == tw, h > th: the reference's randint(0, 0) throws here
    assert (int(r["y1"]), int(r["x1"])) == (8, 0)
    r = sp.record(56, 40, th, tw)                       # stored portrait: the logical frame is 40 x 56
    assert int(r["flags"]) == D.TRANSPOSE and (int(r["y1"]), int(r["x1"])) == (8, 8)
    with pytest.raises(D.ClipReadError, match="too small"):
        sp.record(31, 48, th, tw)


# ---- sources -----------------------------------------------------------------------------------------------------------------------
def test_sources_png_npy_transpose_and_pack_clips(tmp_path):
    clips, lst = write_png_clips(tmp_path, 2, 10, 40, 56)
    paths = D.parse_counted_list(lst.read_text().splitlines())
    assert [len(p) for p in paths] == [10, 10]
    for c in range(2):
        for k in (0, 9):
            assert np.array_equal(D.frame_source(paths[c][k]), clips[c][k])
    np.save(str(tmp_path / "x.npy"), clips[0])
    fr = D.frame_source(str(tmp_path / "x.npy") + "#7")
    assert np.array_equal(fr, clips[0][7])
    buf = np.zeros(4 * 40 * 56 * 3, np.uint8)
    assert D.read_frame_into(paths[1][3], buf, 0, 2, 40 * 56 * 3) == (40, 56)
    assert np.array_equal(buf[2 * 40 * 56 * 3:3 * 40 * 56 * 3].reshape(40, 56, 3), clips[1][3]) and not buf[:2 * 40 * 56 * 3].any()
    with pytest.raises(D.ClipReadError, match="larger than"):
        D.read_frame_into(paths[1][3], buf, 0, 0, 100)
    with pytest.raises(D.ClipReadError, match="missing.png"):
        D.frame_source(str(tmp_path / "missing.png"))
    # a stored h > w frame: the logical frame is its transpose, and the yardstick crops that
    tall = np.ascontiguousarray(clips[0][:3].swapaxes(1, 2))          # stored 56 x 40
    assert np.array_equal(D.logical_frames(tall), clips[0][:3])
    sp = D.plan_sample(0, "vimeo", list("abcdefg"), np.full(D.N_DRAWS, 0.3), 2, "RANDOM", 32, 48)
    a = D.augment_host(tall, sp.record(56, 40, 32, 48), IMAGENET_MEAN, IMAGENET_STD, (32, 48))
    b = D.augment_host(clips[0][:3], sp.record(40, 56, 32, 48), IMAGENET_MEAN, IMAGENET_STD, (32, 48))
    assert np.array_equal(a, b)
    # pack_clips.py: the packed list reads back the PNG frames, through the CLI
    out_list = tmp_path / "packed.txt"
    subprocess.run([sys.executable, os.path.join(ROOT, "superslomo-videointerpolation-pytorch_amd", "scripts", "utils", "pack_clips.py"),
                    str(lst), str(tmp_path / "packed"), str(out_list)], check=True, capture_output=True)
    packed = D.parse_counted_list(out_list.read_text().splitlines())
    assert [len(p) for p in packed] == [10, 10] and packed[1][4].endswith("clip_00001.npy#4")
    for c in range(2):
        for k in range(10):
            assert np.array_equal(D.frame_source(packed[c][k]), clips[c][k])


def test_host_batches_read_what_the_plans_name(tmp_path):
    clips, _ = write_png_clips(tmp_path, 5, 12, 40, 56)
    cfg = make_cfg(tmp_path, size=(40, 56), batch=2, crop=(32, 48))
    ld = D.ClipLoader(cfg, "TRAIN", None, 0, 1, seed=9, n_workers=3)
    n = 0
    for plans, table, frames, t in ld.host_batches(0):
        for sp, r, fr, tt in zip(plans, table, frames, t):
            want = np.stack([D.frame_source(p) for p in sp.paths])
            assert np.array_equal(fr, want) and np.array_equal(want[0], clips[sp.index][int(os.path.basename(sp.paths[0])[:4])])
            assert tt.tolist() == [np.float32(sp.t)] and 0 < sp.t < 1 and r["offset"] % 256 == 0
            n += 1
    assert n == 4


# ---- the yardstick against float64 -------------------------------------------------------------------------------------------------
def reference64(frames, rec, th, tw):
    """The definition of include/ssm_hip.h evaluated in float64, pixel by pixel in plain loops over taps."""
    f = frames.swapaxes(1, 2) if int(rec["flags"]) & D.TRANSPOSE else frames
    y1, x1 = int(rec["y1"]), int(rec["x1"])
    c = f[:, y1:y1 + th, x1:x1 + tw].astype(np.float64)
    if int(rec["flags"]) & D.HFLIP:
        c = c[:, :, ::-1]
    if int(rec["flags"]) & D.AFFINE:
        a = np.asarray(rec["a"], dtype=np.float64)
        s = np.zeros_like(c)
        for y in range(th):
            for x in range(tw):
                u, v = a[0] * x + a[1] * y + a[2], a[3] * x + a[4] * y + a[5]
                i, j = int(np.floor(u)), int(np.floor(v))
                for dy in (0, 1):
                    for dx in (0, 1):
                        if 0 <= j + dy < th and 0 <= i + dx < tw:
                            wgt = (u - i if dx else 1 - (u - i)) * (v - j if dy else 1 - (v - j))
                            s[:, y, x] += wgt * c[:, j + dy, i + dx]
        c = s
    out = (c / 255.0 - np.array(IMAGENET_MEAN)) / np.array(IMAGENET_STD)
    return out.transpose(0, 3, 1, 2)


@pytest.mark.parametrize("stored,flags", [((40, 56), 0), ((40, 56), D.HFLIP), ((56, 40), D.TRANSPOSE), ((56, 40), D.TRANSPOSE | D.HFLIP)])
def test_yardstick_integer_mode_against_float64(stored, flags):
    fr = frames_rgb(3, stored[0], stored[1], 4)
    rec = np.zeros((), D.RECORD)
    rec["hs"], rec["ws"], rec["flags"], rec["y1"], rec["x1"] = stored[0], stored[1], flags, 5, 3
    got = D.augment_host(fr, rec, IMAGENET_MEAN, IMAGENET_STD, (32, 47))
    want = reference64(fr, rec, 32, 47)
    err = np.abs(got.astype(np.float64) - want).max()
    print("integer mode: max |fp32 - fp64| = %.3e (bar %.3e)" % (err, BAR_INT))
    assert got.dtype == np.float32 and got.shape == (3, 3, 32, 47) and err <= BAR_INT


@pytest.mark.parametrize("theta,centre", [(-5.0, (10, 20)), (0.7, (0, 0)), (5.0, (31, 47)), (3.3, (16, 0))])
@pytest.mark.parametrize("flags", [0, D.HFLIP])
def test_yardstick_affine_mode_against_float64(theta, centre, flags):
    th, tw = 32, 48
    fr = frames_rgb(2, 40, 56, 6)
    rec = np.zeros((), D.RECORD)
    rec["hs"], rec["ws"], rec["flags"], rec["y1"], rec["x1"] = 40, 56, flags | D.AFFINE, 4, 7
    rec["a"] = D.rotation_inverse(centre[1], centre[0], theta)
    a = np.abs(np.asarray(rec["a"], dtype=np.float64))
    du = 4 * U * (a[0] * (tw - 1) + a[1] * (th - 1) + a[2])
    dv = 4 * U * (a[3] * (tw - 1) + a[4] * (th - 1) + a[5])
    bar = (255.0 * (du + dv) + 12 * U * 255.0) / 255.0 / 0.224 + BAR_INT
    got = D.augment_host(fr, rec, IMAGENET_MEAN, IMAGENET_STD, (th, tw))
    want = reference64(fr, rec, th, tw)
    err = np.abs(got.astype(np.float64) - want).max()
    print("affine theta %.1f centre %s: max |fp32 - fp64| = %.3e (bar %.3e)" % (theta, centre, err, bar))
    assert err <= bar
    black = (0.0 - np.array(IMAGENET_MEAN)) / np.array(IMAGENET_STD)
    assert theta == 0.7 or np.isclose(got[0, :, 0, 0], black, atol=1e-6).all() or np.isclose(got[0, :, -1, -1], black, atol=1e-6).all() or \
        np.isclose(got[0, :, 0, -1], black, atol=1e-6).all() or np.isclose(got[0, :, -1, 0], black, atol=1e-6).all(), "a rotated crop shows the border"


def test_rotation_inverse_is_the_inverse_of_the_rotation_matrix():
    cx, cy, theta = 13, 29, 4.0
    inv = D.rotation_inverse(cx, cy, theta).astype(np.float64).reshape(2, 3)
    t = np.deg2rad(theta)
    a, b = np.cos(t), np.sin(t)
    m = np.array([[a, b, (1 - a) * cx - b * cy], [-b, a, b * cx + (1 - a) * cy], [0, 0, 1]])
    assert np.abs(np.vstack([inv, [0, 0, 1]]) @ m - np.eye(3)).max() < 1e-5
    assert np.allclose(inv @ np.array([cx, cy, 1.0]), [cx, cy], atol=1e-5)          # the centre stays put
    ident = D.rotation_inverse(7, 9, 0.0)
    assert ident.tolist() == [1.0, 0.0, 0.0, 0.0, 1.0, 0.0] and not np.signbit(ident).any()


def test_affine_identity_equals_integer_mode_in_the_yardstick():
    fr = frames_rgb(3, 40, 56, 8)
    rec = np.zeros((), D.RECORD)
    rec["hs"], rec["ws"], rec["flags"], rec["y1"], rec["x1"] = 40, 56, D.HFLIP, 2, 6
    a = D.augment_host(fr, rec, IMAGENET_MEAN, IMAGENET_STD, (32, 48))
    rec["flags"] = D.HFLIP | D.AFFINE
    rec["a"] = D.rotation_inverse(5, 5, 0.0)
    assert np.array_equal(a, D.augment_host(fr, rec, IMAGENET_MEAN, IMAGENET_STD, (32, 48)))


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------
def test_entry_point_is_declared_bound_and_checks_its_arguments_on_the_host():
    from ssm_amd import hipbind as hb
    hdr = open(os.path.join(ROOT, "include", "ssm_hip.h")).read()
    assert "int ssm_clip_batch_from_u8_fwd(" in hdr and "ssm_clip_record" in hdr
    assert "ssm_clip_batch_from_u8_fwd" in hb.SIGNATURES and hasattr(hb.load(), "ssm_clip_batch_from_u8_fwd")
    # RECORD is the one Python statement of ssm_clip_record's layout (csrc/ssm_data.hip static_asserts the 64 bytes): offsets as the C struct's
    assert D.RECORD.itemsize == 64
    assert {n: D.RECORD.fields[n][1] for n in D.RECORD.names} == {"offset": 0, "hs": 8, "ws": 12, "flags": 16, "y1": 20, "x1": 24, "a": 28, "reserved": 52}
    for name, val in (("TRANSPOSE", D.TRANSPOSE), ("HFLIP", D.HFLIP), ("AFFINE", D.AFFINE)):
        assert "#define SSM_CLIP_%s %d\n" % (name, val) in hdr
    rc = hb.load().ssm_clip_batch_from_u8_fwd(None, 64, None, None, None, None, 1, 3, 2, 8, 8, None, None, None)          # refused on the host: no launch
    assert rc == -1 and b"null" in hb.load().ssm_last_error_string()
