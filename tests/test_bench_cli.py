"""bench.py's command line: what a plain run leaves out, what --full puts back,
and --dump-outputs (a fixed, seeded sample; the same files from run to run; the
dumped frames are the reference's frames of the dumped decoded bytes)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

import bench


def _parse(monkeypatch, *argv):
    monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
    return bench.parse()


def test_plain_run_leaves_the_side_legs_out(monkeypatch):
    a = _parse(monkeypatch, "--gpus", "1", "--steps", "7", "--warmup", "2")
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 2, False, None)
    assert a.no_cpu_baseline and a.no_host_inclusive and a.no_verify


def test_full_run_keeps_them_and_their_switches(monkeypatch):
    a = _parse(monkeypatch, "--full", "--dump-outputs", "d")
    assert a.full and a.dump_outputs == "d"
    assert not (a.no_cpu_baseline or a.no_host_inclusive or a.no_verify)
    a = _parse(monkeypatch, "--full", "--no-cpu-baseline")
    assert a.no_cpu_baseline and not a.no_verify


@pytest.mark.parametrize("sizes", [np.full(1 << 12, 4096, np.uint32), np.full(40, 1 << 20, np.uint32),
                                   np.full(3, 100, np.uint32),
                                   np.tile(np.array([100, 4096, 65536], np.uint32), 5000)])
def test_dump_sample_is_fixed_and_bounded(sizes):
    per_value, idx = bench.dump_sample(sizes)
    again = bench.dump_sample(sizes.copy())
    assert np.array_equal(per_value, again[0]) and np.array_equal(idx, again[1])
    assert np.array_equal(per_value, np.arange(len(sizes)))          # below the per-value cap: all of them
    assert len(idx) >= 1 and np.array_equal(idx, np.unique(idx))
    raw = int(sizes[idx].astype(np.int64).sum())
    # whole values up to the byte budget: the one that crosses it is the last taken
    assert raw - int(sizes.max()) < bench.DUMP_SAMPLE_BYTES or len(idx) == 1
    assert raw >= min(bench.DUMP_SAMPLE_BYTES, int(sizes.astype(np.int64).sum()))


def test_dump_sample_caps_the_per_value_arrays(monkeypatch):
    monkeypatch.setattr(bench, "DUMP_PER_VALUE", 1000)
    per_value, idx = bench.dump_sample(np.full(5000, 100, np.uint32))
    assert len(per_value) == 1000 and np.array_equal(per_value, np.unique(per_value)) and per_value.max() < 5000
    assert set(idx) <= set(per_value)


def test_write_dump_is_float_and_exact(tmp_path):
    arrays = {"small": np.array([0, 255, (1 << 24) - 1], np.uint32), "wide": np.array([1, (1 << 40) + 1], np.uint64),
              "status": np.array([-22, 0], np.int32)}
    bench.write_dump(str(tmp_path / "d"), arrays)
    got = {k: np.load(tmp_path / "d" / (k + ".npy")) for k in arrays}
    assert (got["small"].dtype, got["wide"].dtype, got["status"].dtype) == (np.float32, np.float64, np.float32)
    for k, a in arrays.items():
        assert np.array_equal(got[k].astype(np.int64), a.astype(np.int64)), k


def _run(tmp_path, name):
    d = tmp_path / name
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
                        "--values", "1024", "--dump-outputs", str(d)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout.strip().splitlines()[-1]), {f[:-4]: np.load(d / f) for f in sorted(os.listdir(d))}


@pytest.mark.gpu
def test_plain_run_dumps_the_same_outputs_every_time(gpu, orc, tmp_path):
    line, a = _run(tmp_path, "a")
    _, b = _run(tmp_path, "b")
    assert line["steps"] == 2 and line["warmup"] == 1 and line["ms_per_step"] > 0 and line["value"] > 0
    assert line["unit"] == "GiB/s" and line["higher_is_better"] is True and line["dtype"] == "u8"
    assert line["metric"] == bench.METRIC
    # a plain run: none of the side legs
    assert line["cpu_baseline"] is None and "host_inclusive" not in line and line["roofline"]["copy_gbs"] is None
    assert line["verify"].startswith("statuses and lengths only")
    assert sorted(a) == sorted(b) == ["compress_status", "decoded_lens", "decompress_status", "frame_lens",
                                      "sample_decoded", "sample_frames", "sample_values"]
    for k in a:
        assert a[k].dtype in (np.float32, np.float64) and np.array_equal(a[k], b[k]), k
    assert sum(v.nbytes for v in a.values()) <= 64_000_000
    n, size = 1024, 4096
    assert not a["compress_status"].any() and not a["decompress_status"].any()
    assert len(a["frame_lens"]) == n and (a["decoded_lens"] == size).all()
    # the sampled values: decoded bytes are whole values, their frames the reference's
    idx = a["sample_values"].astype(np.int64)
    dec = a["sample_decoded"].astype(np.uint8).reshape(len(idx), size)
    frames, pos = a["sample_frames"].astype(np.uint8), 0
    for k, i in enumerate(idx):
        want = orc.frame(dec[k].tobytes())
        assert len(want) == int(a["frame_lens"][i])
        assert frames[pos:pos + len(want)].tobytes() == want, i
        pos += len(want)
    assert pos == len(frames)
