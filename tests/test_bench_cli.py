"""bench.py's command line and the flattening behind --dump-outputs (CPU only)."""
import sys

import numpy as np

import pyoracle as po


def parse(argv):
    import bench
    old = sys.argv
    sys.argv = ["bench.py"] + argv
    try:
        return bench.parse()
    finally:
        sys.argv = old


def test_plain_run_is_the_default():
    a = parse(["--gpus", "1", "--steps", "7", "--warmup", "3"])
    assert (a.gpus, a.steps, a.warmup) == (1, 7, 3)
    assert a.full is False and a.dump_outputs is None
    b = parse(["--full", "--dump-outputs", "somewhere"])
    assert b.full is True and b.dump_outputs == "somewhere"


def test_leaves_cover_every_field_and_skip_padding():
    import bench
    obs = np.zeros(3, dtype=po.OBS)
    obs.view(np.uint8)[:] = 0xFF                           # padding bytes included
    obs["shared"]["current_resources"] = 1.5
    got = list(bench.leaves(obs))
    assert [nm for nm, _ in got] == [nm for nm, _ in po.leaves(obs)]
    cols = sum(x[0].size for _, x in got)
    assert cols == 48 * 48 * 7 + 1 + 3 + 18 + 4 * (5 * 21 + 3 * 22 + 7 + 19)   # api.h:67-129, no padding
    rows = np.concatenate([x.reshape(3, -1).astype(np.float32) for _, x in got], axis=1)
    assert rows.shape == (3, cols) and rows.dtype == np.float32
    assert set(np.unique(rows)) == {1.0, 1.5, 255.0}       # bools read as 1, u8 as 255, the floats kept
