import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "superslomo-videointerpolation-pytorch_amd")
for p in (ROOT, PKG, os.path.join(PKG, "scripts")):
    if p not in sys.path:
        sys.path.insert(0, p)

GOLDEN = os.path.join(ROOT, "tests", "golden")


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (run with -m gpu)")
    # The CPU oracle (torch fp32 on the host) is what most of the suite's wall time goes to.  A GPU box exposes all 256 logical CPUs of its
    # host to a job that owns a 16-CPU share of it: torch's default (one thread per core it can see) oversubscribes that share 8x and a
    # 736x1280 stage-1 pass takes 13 s instead of 2.9 (bench.py's thread sweep, cpu_baseline.thread_sweep_c2_stage1_seconds).  16 threads
    # at most; fewer where the affinity mask is smaller (8 in the build container).
    import torch
    torch.set_num_threads(max(1, min(16, len(os.sched_getaffinity(0)))))


# Collection order (the driver runs `pytest -x`): kernel-level suites that hold every forced tile configuration of a kernel family to the
# oracle run first, model-level suites at small sizes next, end-to-end cases at a BASELINE workload size (720p / 4K / config 3-5) last -
# a marginal big-shape assertion must never hide a kernel suite.  Module-scoped fixtures stay grouped: the key is (tier, suite rank inside the kernel tier, original index).
_KERNEL_SUITES = ("test_hip_wino7", "test_hip_wino5", "test_hip_wino4", "test_hip_wino1d", "test_hip_wino", "test_hip_overshoot", "test_hip_conv_f32", "test_hip_ops", "test_hip_pack_batch", "test_hip_threads",
                  "test_frames_eval", "test_hip_rccl_world1", "test_hip_conv16", "test_hip_conv16_q8")   # the headline's kernels first
_BIG_SHAPE = ("720p", "4k", "config3", "config4", "config5")


def _tier(item):
    mod = os.path.splitext(os.path.basename(str(item.fspath)))[0]
    if item.get_closest_marker("gpu") is None:
        return 0
    if any(tag in item.name.lower() for tag in _BIG_SHAPE):
        return 3
    return 1 if mod in _KERNEL_SUITES else 2


def pytest_collection_modifyitems(config, items):
    order = {id(it): i for i, it in enumerate(items)}

    def suite(it):
        mod = os.path.splitext(os.path.basename(str(it.fspath)))[0]
        return _KERNEL_SUITES.index(mod) if mod in _KERNEL_SUITES else len(_KERNEL_SUITES)
    items.sort(key=lambda it: (_tier(it), suite(it) if _tier(it) == 1 else 0, order[id(it)]))


@pytest.fixture(scope="session")
def golden():
    import numpy as np

    cache = {}

    def load(name):
        if name not in cache:
            cache[name] = dict(np.load(os.path.join(GOLDEN, name + ".npz")))
            # a fixture too large for one archive continues in <name>.part2.npz, <name>.part3.npz, ... (make_golden.save_fixture)
            i = 2
            while os.path.exists(os.path.join(GOLDEN, "%s.part%d.npz" % (name, i))):
                cache[name].update(np.load(os.path.join(GOLDEN, "%s.part%d.npz" % (name, i))))
                i += 1
        return cache[name]

    return load
