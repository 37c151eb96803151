"""The training ingest on the GPU: the kernel of csrc/ssm_data.hip against its numpy float32 yardstick (ssm_amd.data.augment_host, itself
held to a float64 evaluation in tests/test_data_cpu.py) - BIT-equal, since kernel and yardstick perform the same rounded fp32 operations
in the same order on the same fp32 constants - and against ssm_frames_from_u8_fwd of host-cropped frames; the loader (ClipLoader) end to
end against records + source + yardstick; scripts/main.py training from a clip list."""
import configparser
import os
import threading
import time

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")


def D():
    from ssm_amd import data
    return data


def mean_std():
    from ssm_amd.weights import IMAGENET_MEAN, IMAGENET_STD
    return IMAGENET_MEAN, IMAGENET_STD


def frames_rgb(n, h, w, seed):
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    base = np.stack([(3 * xx + 5 * yy) % 256, (7 * xx + 2 * yy + 40) % 256, (xx * yy + 11) % 256], -1)
    return np.stack([((base + 9 * i + rng.randint(0, 24, base.shape)) % 256).astype(np.uint8) for i in range(n)])


def record(hs, ws, y1, x1, flags=0, a=None):
    r = np.zeros((), D().RECORD)
    r["hs"], r["ws"], r["y1"], r["x1"], r["flags"] = hs, ws, y1, x1, flags
    if a is not None:
        r["a"] = a
    return r


def run_kernel(samples, th, tw, n_in, skew=0):
    """samples: [(frames [F,Hs,Ws,3] uint8, record)].  Lays the staging buffer out (table, then the samples, the first one `skew` bytes
    past a 256-byte boundary), runs the kernel, returns (input, target) as numpy and the table."""
    d = D()
    b, f = len(samples), samples[0][0].shape[0]
    table = np.zeros(b, d.RECORD)
    off = 256 * ((b * 64 + 255) // 256) + skew
    chunks = []
    for i, (fr, r) in enumerate(samples):
        table[i] = r
        table[i]["offset"] = off
        chunks.append((off, np.ascontiguousarray(fr).reshape(-1)))
        off += fr.size + (-fr.size) % 4 + 4 * (i % 2)          # samples start at assorted multiples of 4
    host = np.zeros(off + (-off) % 4, np.uint8)
    host[:b * 64] = table.view(np.uint8)
    for o, c in chunks:
        host[o:o + c.size] = c
    staging = torch.from_numpy(host).to(DEV)
    inp = torch.full((b, n_in, 3, th, tw), 7.0, device=DEV)
    tgt = torch.full((b, f - n_in, 3, th, tw), 7.0, device=DEV)
    d.clip_batch_from_u8(staging, table, inp, tgt)
    torch.cuda.synchronize()
    return inp.cpu().numpy(), tgt.cpu().numpy(), table


def yardstick(samples, th, tw, n_in):
    d = D()
    mean, std = mean_std()
    x = np.stack([d.augment_host(fr, r, mean, std, (th, tw)) for fr, r in samples])
    return x[:, :n_in], x[:, n_in:]


def assert_bit_equal(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype == np.float32, what
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), "%s: %d of %d values differ, max |d| %.3e" % (
        what, int((got.view(np.uint32) != want.view(np.uint32)).sum()), got.size, float(np.abs(got - want).max()))


# (stored size, crop, y1, x1, flags): every x1 % 4 at odd y1, widths with tw % 4 != 0, the whole frame, mirrored, transposed
INT_CASES = [((96, 128), (32, 64), 1, 0, 0), ((96, 128), (32, 64), 3, 1, 0), ((96, 128), (32, 64), 5, 2, 0), ((96, 128), (32, 64), 7, 3, 0),
             ((96, 128), (33, 45), 9, 5, 0), ((96, 128), (31, 46), 1, 82, 2), ((96, 128), (30, 47), 11, 7, 2), ((64, 112), (64, 112), 0, 0, 0),
             ((64, 112), (64, 112), 0, 0, 2), ((96, 128), (32, 64), 3, 9, 2), ((128, 96), (32, 64), 5, 3, 1), ((128, 96), (31, 45), 64, 83, 3),
             ((128, 96), (96, 128), 0, 0, 1), ((40, 300), (8, 257), 31, 43, 2)]


@pytest.mark.parametrize("stored,crop,y1,x1,flags", INT_CASES)
@pytest.mark.parametrize("nf", [(3, 2), (7, 4)])
def test_integer_mode_equals_the_yardstick(stored, crop, y1, x1, flags, nf):
    f, n_in = nf
    samples = [(frames_rgb(f, stored[0], stored[1], 3 + b), record(stored[0], stored[1], y1, x1, flags)) for b in range(2)]
    for skew in (0, 4):
        inp, tgt, _ = run_kernel(samples, crop[0], crop[1], n_in, skew)
        wi, wt = yardstick(samples, crop[0], crop[1], n_in)
        assert_bit_equal(inp, wi, "input")
        assert_bit_equal(tgt, wt, "target")


def test_a_batch_mixes_source_sizes_and_flags():
    d = D()
    samples = [(frames_rgb(3, 96, 128, 1), record(96, 128, 13, 31, 0)), (frames_rgb(3, 64, 112, 2), record(64, 112, 0, 47, d.HFLIP)),
               (frames_rgb(3, 112, 64, 3), record(112, 64, 0, 41, d.TRANSPOSE)), (frames_rgb(3, 96, 128, 4), record(96, 128, 31, 63, d.HFLIP)),
               (frames_rgb(3, 64, 112, 5), record(64, 112, 0, 2, d.AFFINE, d.rotation_inverse(20, 30, 3.0)))]
    inp, tgt, _ = run_kernel(samples, 64, 64, 2)
    wi, wt = yardstick(samples, 64, 64, 2)
    assert_bit_equal(inp, wi, "input")
    assert_bit_equal(tgt, wt, "target")


@pytest.mark.parametrize("flip", [False, True])
def test_integer_mode_equals_frames_from_u8_of_host_cropped_frames(flip):
    from ssm_amd.frames import frames_from_u8
    d = D()
    th, tw = 64, 96                                     # multiples of 32: frames_from_u8 pads nothing
    fr = frames_rgb(3, 96, 128, 11)
    inp, tgt, _ = run_kernel([(fr, record(96, 128, 17, 29, d.HFLIP if flip else 0))], th, tw, 2)
    crop = fr[:, 17:17 + th, 29:29 + tw]
    crop = np.ascontiguousarray(crop[:, :, ::-1] if flip else crop)
    want = frames_from_u8(torch.from_numpy(crop).to(DEV)).cpu().numpy()
    assert want.shape == (3, 3, th, tw)
    assert_bit_equal(np.concatenate([inp[0], tgt[0]]), want, "frames_from_u8")


@pytest.mark.parametrize("theta", [-5.0, 0.7, 5.0])
@pytest.mark.parametrize("centre", [(20, 30), (0, 0), (47, 63), (0, 63)])
def test_affine_mode_equals_the_yardstick(theta, centre):
    d = D()
    th, tw = 48, 64
    for flags, stored, tw_ in ((d.AFFINE, (96, 128), tw), (d.AFFINE | d.HFLIP, (96, 128), tw - 3), (d.AFFINE | d.TRANSPOSE, (128, 96), tw)):
        cx = min(centre[1], tw_ - 1)
        samples = [(frames_rgb(3, stored[0], stored[1], 21), record(stored[0], stored[1], 7, 9, flags, d.rotation_inverse(cx, centre[0], theta)))]
        inp, tgt, _ = run_kernel(samples, th, tw_, 2)
        wi, wt = yardstick(samples, th, tw_, 2)
        assert_bit_equal(inp, wi, "input (flags %d)" % flags)
        assert_bit_equal(tgt, wt, "target (flags %d)" % flags)


def test_affine_identity_equals_integer_mode():
    d = D()
    fr = frames_rgb(3, 96, 128, 31)
    for flags in (0, d.HFLIP):
        a, at, _ = run_kernel([(fr, record(96, 128, 5, 7, flags))], 48, 62, 2)
        b, bt, _ = run_kernel([(fr, record(96, 128, 5, 7, flags | d.AFFINE, d.rotation_inverse(11, 13, 0.0)))], 48, 62, 2)
        assert_bit_equal(b, a, "input")
        assert_bit_equal(bt, at, "target")


def test_argument_errors_launch_nothing():
    import ctypes
    from ssm_amd import hipbind as hb
    from ssm_amd.frames import _f3
    d = D()
    lib = hb.load()
    mean, std = _f3((0.5,) * 3), _f3((0.25,) * 3)
    hs, ws, f, th, tw = 16, 24, 3, 8, 12
    nbytes = 256 + f * hs * ws * 3
    staging = torch.zeros(nbytes, dtype=torch.uint8, device=DEV)
    inp = torch.full((1, 2, 3, th, tw), 7.0, device=DEV)
    tgt = torch.full((1, 1, 3, th, tw), 7.0, device=DEV)

    def call(rec=None, upload=False, **kw):
        r = record(hs, ws, 2, 3)
        r["offset"] = 256
        for k, v in (rec or {}).items():
            r[k] = v
        table = np.array([r], d.RECORD)
        a = dict(frames=staging.data_ptr(), nbytes=nbytes, tdev=staging.data_ptr(), thost=table.ctypes.data_as(ctypes.c_void_p), inp=inp.data_ptr(),
                 tgt=tgt.data_ptr(), B=1, F=f, n_in=2, th=th, tw=tw, mean=mean, std=std)
        a.update(kw)
        if upload:                                      # only the calls meant to run put their record where the kernel reads it
            staging[:64].copy_(torch.from_numpy(table.view(np.uint8).copy()))
        hb.check(lib.ssm_clip_batch_from_u8_fwd(a["frames"], a["nbytes"], a["tdev"], a["thost"], a["inp"], a["tgt"], a["B"], a["F"], a["n_in"],
                                                a["th"], a["tw"], a["mean"], a["std"], hb.stream_ptr()))

    bad = [(dict(frames=None), "null"), (dict(tdev=None), "null"), (dict(thost=None), "null"), (dict(inp=None), "null"), (dict(tgt=None), "null"),
           (dict(mean=None), "null"), (dict(std=None), "null"), (dict(B=0), "geometry"), (dict(F=0), "geometry"), (dict(th=0), "geometry"),
           (dict(tw=0), "geometry"), (dict(nbytes=0), "geometry"), (dict(n_in=0), "n_in"), (dict(n_in=3), "n_in"), (dict(F=1, n_in=1), "n_in"),
           (dict(B=21846, F=3), "geometry"),          # B F = 65538 > 65535 (refused before the table is read)
           (dict(th=65536, tw=1 << 19), "geometry"),          # th ceil(tw / 4) = 2^33 > 2^31 - 1
           (dict(nbytes=nbytes - 1), "leave the buffer"), (dict(F=4, n_in=2), "leave the buffer")]
    bad_rec = [(dict(y1=-1), "leaves"), (dict(x1=-1), "leaves"), (dict(y1=hs - th + 1), "leaves"), (dict(x1=ws - tw + 1), "leaves"),
               (dict(flags=1, x1=ws - tw), "leaves"),          # x1 = 12 fits the stored 24 columns, not the 16 of the transposed frame
               (dict(hs=0), "bad record"), (dict(ws=-4), "bad record"), (dict(offset=-256), "bad record"), (dict(flags=8), "bad record"),
               (dict(offset=260), "leave the buffer")]
    for kw, pat in bad:
        with pytest.raises(RuntimeError, match=pat):
            call(**kw)
    for rec, pat in bad_rec:
        with pytest.raises(RuntimeError, match=pat):
            call(rec=rec)
    torch.cuda.synchronize()
    assert float(inp.min()) == float(inp.max()) == 7.0 and float(tgt.min()) == float(tgt.max()) == 7.0, "a refused call wrote"
    call(upload=True)                                   # ... and the good call runs
    call(rec=dict(y1=hs - th, x1=ws - tw), upload=True)            # the last offsets are inside
    torch.cuda.synchronize()
    assert float(inp.max()) < 7.0


def test_a_buffer_that_is_not_dword_aligned_reads_single_bytes():
    """A `frames` pointer (or size) that is no multiple of 4 takes the byte loads everywhere: straight through the C ABI, since the Python
    wrapper always passes an aligned tensor.  The table stays where it is aligned; offsets count from `frames`."""
    import ctypes
    from ssm_amd import hipbind as hb
    from ssm_amd.frames import _f3
    d = D()
    mean, std = mean_std()
    hs, ws, f, th, tw = 40, 56, 3, 32, 48
    fr = frames_rgb(f, hs, ws, 77)
    for shift, pad in ((1, 0), (2, 0), (3, 0), (0, 1)):          # misaligned base; aligned base with a size that is not a multiple of 4
        for flags in (0, d.HFLIP):
            r = record(hs, ws, 5, 3, flags)
            r["offset"] = 256 - shift
            table = np.array([r], d.RECORD)
            host = np.zeros(256 + fr.size + pad, np.uint8)
            host[:64] = table.view(np.uint8)
            host[256:256 + fr.size] = fr.reshape(-1)
            staging = torch.from_numpy(host).to(DEV)
            inp = torch.full((1, 2, 3, th, tw), 7.0, device=DEV)
            tgt = torch.full((1, 1, 3, th, tw), 7.0, device=DEV)
            hb.check(hb.load().ssm_clip_batch_from_u8_fwd(staging.data_ptr() + shift, host.size - shift, staging.data_ptr(),
                                                          table.ctypes.data_as(ctypes.c_void_p), inp.data_ptr(), tgt.data_ptr(), 1, f, 2, th, tw,
                                                          _f3(mean), _f3(std), hb.stream_ptr()))
            torch.cuda.synchronize()
            want = d.augment_host(fr, r, mean, std, (th, tw))
            assert_bit_equal(inp.cpu().numpy()[0], want[:2], "input (shift %d, pad %d)" % (shift, pad))
            assert_bit_equal(tgt.cpu().numpy()[0], want[2:], "target (shift %d, pad %d)" % (shift, pad))


# ---- the loader --------------------------------------------------------------------------------------------------------------------
def make_cfg(tmp_path, batch=2, crop=(32, 48), size=(96, 128)):
    from ssm_amd.config import CONFIG_DIR
    cfg = configparser.RawConfigParser()
    cfg.read(os.path.join(CONFIG_DIR, "superslomo_original.ini"))
    cfg.set("DATA", "DATASET", "ADOBE")
    cfg.set("ADOBE_DATA", "TRAINPATHS", str(tmp_path / "train.txt"))
    cfg.set("ADOBE_DATA", "H_IN", str(size[0]))
    cfg.set("ADOBE_DATA", "W_IN", str(size[1]))
    for k, v in (("BATCH_SIZE", batch), ("CROP_IMH", crop[0]), ("CROP_IMW", crop[1])):
        cfg.set("TRAIN", k, str(v))
    return cfg


def write_clips(tmp_path, n_clips=6, n_frames=12, h=96, w=128):
    from PIL import Image
    from ssm_amd.weights import synthetic_frames_u8
    lines = ["%d" % n_clips]
    for c in range(n_clips):
        fr = synthetic_frames_u8(n_frames, h, w, seed=50 + c).permute(0, 2, 3, 1).contiguous().numpy()
        (tmp_path / ("clip%02d" % c)).mkdir()
        lines.append("%d" % n_frames)
        for k in range(n_frames):
            p = str(tmp_path / ("clip%02d" % c) / ("%04d.png" % k))
            Image.fromarray(fr[k]).save(p)
            lines.append(p)
    (tmp_path / "train.txt").write_text("\n".join(lines) + "\n")
    return lines


def expected_batches(cfg, epoch, seed, **kw):
    """[(input, target, t)] float32 numpy of an epoch: records + source + yardstick, host only."""
    ld = D().ClipLoader(cfg, "TRAIN", None, 0, 1, seed=seed, n_workers=2, **kw)
    out = []
    for plans, table, frames, t in ld.host_batches(epoch):
        wi, wt = ld.yardstick(table, frames)
        out.append((wi, wt, t.reshape(t.shape + (1, 1, 1))))
    return out


def loader_threads():
    return [t for t in threading.enumerate() if t.name.startswith("clip-loader")]


@pytest.mark.parametrize("aug", [False, True])
def test_loader_equals_records_source_and_yardstick(tmp_path, aug):
    write_clips(tmp_path)
    cfg = make_cfg(tmp_path)
    kw = dict(flip=aug, rotate=aug)
    seen = {}
    for nw in (1, 4):
        ld = D().ClipLoader(cfg, "TRAIN", DEV, 0, 1, seed=7, n_workers=nw, **kw)
        assert len(ld) == 3
        for epoch in (0, 1):
            want = expected_batches(cfg, epoch, 7, **kw)
            n = 0
            for (inp, tgt, t), (wi, wt, wtt) in zip(ld, want):          # compared when consumed
                assert tuple(inp.shape) == (2, 2, 3, 32, 48) and tuple(tgt.shape) == (2, 1, 3, 32, 48) and tuple(t.shape) == (2, 1, 1, 1, 1)
                assert_bit_equal(inp.cpu().numpy(), wi, "epoch %d batch %d input" % (epoch, n))
                assert_bit_equal(tgt.cpu().numpy(), wt, "epoch %d batch %d target" % (epoch, n))
                assert np.array_equal(t.cpu().numpy(), wtt)
                seen.setdefault((epoch, n), []).append((inp.cpu().numpy().tobytes(), tgt.cpu().numpy().tobytes()))
                n += 1
            assert n == 3 and ld.epoch == epoch + 1
        assert not loader_threads()
    assert len(seen) == 6 and all(len(v) == 2 and v[0] == v[1] for v in seen.values()), "1 and 4 workers must give the same batches"
    assert seen[0, 0] != seen[1, 0]


def test_a_slot_is_not_reused_while_its_batch_is_held(tmp_path):
    write_clips(tmp_path, n_clips=26)
    cfg = make_cfg(tmp_path)
    depth = 3
    ld = D().ClipLoader(cfg, "TRAIN", DEV, 0, 1, seed=1, n_workers=4, depth=depth)
    want = expected_batches(cfg, 0, 1)
    assert len(want) == 13 >= 4 * depth
    prev = None
    n = 0
    for (inp, tgt, t), (wi, wt, _) in zip(ld, want):          # no reference to a batch outlives the request for the next one
        if prev is not None:                            # just after the next batch was requested: the clone taken first must still be right
            assert_bit_equal(prev[0].cpu().numpy(), prev[1], "clone of batch %d" % (n - 1))
        assert_bit_equal(inp.cpu().numpy(), wi, "batch %d" % n)          # before asking for the next: nothing later has written this slot
        assert_bit_equal(tgt.cpu().numpy(), wt, "batch %d target" % n)
        prev = (inp.clone(), wi)
        del inp, tgt, t
        n += 1
    assert n == 13


def test_memory_is_flat_in_epoch_length(tmp_path, monkeypatch):
    pins = []          # every pinning of host memory during a run: (bytes) per torch.Tensor.pin_memory call
    real_pin = torch.Tensor.pin_memory

    def counting_pin(self, *a, **kw):
        pins.append(self.numel() * self.element_size())
        return real_pin(self, *a, **kw)

    monkeypatch.setattr(torch.Tensor, "pin_memory", counting_pin)
    write_clips(tmp_path, n_clips=80, n_frames=9, h=64, w=96)
    cfg = make_cfg(tmp_path, crop=(32, 48), size=(64, 96))
    peaks, pinned = [], []
    for n_clips in (16, 16, 80):                        # 8, 8 and 40 batches of 2
        lines = (tmp_path / "train.txt").read_text().splitlines()
        (tmp_path / "short.txt").write_text("\n".join(lines[1:1 + 10 * n_clips]) + "\n")
        cfg.set("ADOBE_DATA", "TRAINPATHS", str(tmp_path / "short.txt"))
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(DEV)
        del pins[:]
        ld = D().ClipLoader(cfg, "TRAIN", DEV, 0, 1, seed=2, n_workers=4)
        n = sum(1 for _ in ld)
        assert n == n_clips // 2
        torch.cuda.synchronize()
        peaks.append(torch.cuda.max_memory_allocated(DEV))
        pinned.append((len(pins), sum(pins)))
        del ld
    print("peak device memory: 8 batches %d B, 40 batches %d B; pinned (calls, bytes) %s, %s" % (peaks[1], peaks[2], pinned[1], pinned[2]))
    assert peaks[2] <= peaks[1]
    assert pinned[2] == pinned[1] and pinned[1][0] == 3 and pinned[1][1] > 0, "host memory is pinned once per slot, whatever the epoch's length"


def test_a_corrupt_png_surfaces_with_its_path_and_ends_the_threads(tmp_path):
    lines = write_clips(tmp_path, n_clips=12)
    cfg = make_cfg(tmp_path)
    ld = D().ClipLoader(cfg, "TRAIN", DEV, 0, 1, seed=4, n_workers=4)
    batches = ld.plan_epoch(0)
    victim = batches[3][1].paths[0]                     # a frame of the fourth batch
    with open(victim, "r+b") as f:
        f.seek(40)
        f.write(b"\x00" * 4000)
    got = 0
    with pytest.raises(D().ClipReadError) as ei:
        for _ in ld:
            got += 1
    assert victim in str(ei.value) and got <= 3
    t0 = time.time()
    while loader_threads() and time.time() - t0 < 5:
        time.sleep(0.05)
    assert not loader_threads(), [t.name for t in loader_threads()]
    torch.cuda.synchronize()
    assert lines


# ---- scripts/main.py ---------------------------------------------------------------------------------------------------------------
def train_ini(tmp_path, **train):
    cfg = make_cfg(tmp_path, batch=2, crop=(64, 64))
    cfg.set("STAGE1", "LOADPREV", "FALSE")
    cfg.set("STAGE2", "LOADPREV", "FALSE")
    cfg.set("STAGE1", "FREEZE", "TRUE")                 # one trainable stage
    cfg.set("STAGE2", "FREEZE", "FALSE")
    for k, v in dict(N_EPOCHS="2", SAVE_EVERY="2", CKPT_DIR=str(tmp_path / "ckpt"), **train).items():
        cfg.set("TRAIN", k, v)
    ini = tmp_path / "train.ini"
    with open(ini, "w") as f:
        cfg.write(f)
    return cfg, ini


def test_main_trains_from_a_clip_list(tmp_path, monkeypatch):
    import main as M
    write_clips(tmp_path)
    cfg, ini = train_ini(tmp_path)
    seen = []

    class Spy(M.ClipLoader):
        def __iter__(self):
            for inp, tgt, t in super().__iter__():
                seen.append((self.epoch - 1, inp.cpu().numpy(), tgt.cpu().numpy(), t.cpu().numpy()))
                yield inp, tgt, t

    losses = []

    class Logged(M.Trainer):
        def train_step(self, *a, **kw):
            out = super().train_step(*a, **kw)
            losses.append(out.cpu().tolist())
            return out

    monkeypatch.setattr(M, "ClipLoader", Spy)
    monkeypatch.setattr(M, "Trainer", Logged)
    ckpt = M.main(["-c", str(ini), "--expt", "e", "--log", str(tmp_path / "t.log"), "--flip"])
    assert ckpt and ckpt.endswith("e_EPOCH_0002.pt") and os.path.exists(ckpt)
    data = torch.load(ckpt, map_location="cpu")
    assert set(data) == {"epoch", "stage1_state_dict", "stage2_state_dict", "self.optimizer", "scheduler"} and data["epoch"] == 2
    assert {int(v["step"]) for v in data["self.optimizer"]["state"].values()} == {6}          # 2 epochs x 3 batches
    # the batches Trainer saw are the loader's yardstick batches of epochs 1 and 2 (main numbers epochs from 1), seed SEED.VALUE
    assert [e for e, *_ in seen] == [1, 1, 1, 2, 2, 2]
    want = expected_batches(cfg, 1, cfg.getint("SEED", "VALUE"), flip=True) + expected_batches(cfg, 2, cfg.getint("SEED", "VALUE"), flip=True)
    for (_, inp, tgt, t), (wi, wt, wtt) in zip(seen, want):
        assert_bit_equal(inp, wi, "input")
        assert_bit_equal(tgt, wt, "target")
        assert np.array_equal(t, wtt)
    assert len(losses) == 6 and all(len(v) == 4 and np.isfinite(v).all() for v in losses)
    assert not loader_threads()


def test_main_synthetic_batches_still_run(tmp_path):
    import main as M
    _, ini = train_ini(tmp_path)                        # no clip list exists: the synthetic path must not look for one
    ckpt = M.main(["-c", str(ini), "--expt", "s", "--log", str(tmp_path / "s.log"), "--synthetic_batches", "2"])
    assert ckpt.endswith("s_EPOCH_0002.pt") and torch.load(ckpt, map_location="cpu")["epoch"] == 2
