"""bench.py --dump-outputs writer: dtype mapping, whole-array vs seeded
sample, and run-to-run determinism of the sampled positions (CPU tensors;
the writer is device-agnostic)."""
import json
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import bench  # noqa: E402


def test_dump_whole_arrays(tmp_path):
    ranks = torch.arange(1000, dtype=torch.float32) / 7
    # u32 labels live in int32 storage: 0xFFFFFFFF (unreached) is -1
    labels = torch.tensor([0, 5, -1, 2 ** 31 - 1, -2 ** 31], dtype=torch.int32)
    d = str(tmp_path / "out")
    bench.dump_outputs(d, {"ranks": ranks, "labels": labels})
    assert sorted(os.listdir(d)) == ["labels.npy", "ranks.npy"]
    r = np.load(os.path.join(d, "ranks.npy"))
    assert r.dtype == np.float32
    np.testing.assert_array_equal(r, ranks.numpy())
    lab = np.load(os.path.join(d, "labels.npy"))
    assert lab.dtype == np.float64
    np.testing.assert_array_equal(
        lab, [0, 5, 0xFFFFFFFF, 2 ** 31 - 1, 2 ** 31])


def test_dump_samples_large_arrays(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_VALUE_BYTES", 4 * 100)
    vec = torch.arange(64 * 50, dtype=torch.float32).view(50, 64)
    d1, d2 = str(tmp_path / "a"), str(tmp_path / "b")
    bench.dump_outputs(d1, {"vectors": vec})
    bench.dump_outputs(d2, {"vectors": vec})
    v = np.load(os.path.join(d1, "vectors.npy"))
    idx = np.load(os.path.join(d1, "vectors_index.npy"))
    assert v.dtype == np.float32 and idx.dtype == np.float64
    assert v.shape == idx.shape == (100,)
    # distinct, ascending, in range (one position per stratum)
    assert (np.diff(idx) > 0).all() and idx.min() >= 0 \
        and idx.max() < vec.numel()
    # values are the flat array at the recorded positions
    np.testing.assert_array_equal(v, idx.astype(np.float32))
    # fixed seed: a second dump samples the same positions
    np.testing.assert_array_equal(
        idx, np.load(os.path.join(d2, "vectors_index.npy")))
    np.testing.assert_array_equal(
        v, np.load(os.path.join(d2, "vectors.npy")))


@pytest.mark.parametrize("dtype", [torch.float64, torch.bfloat16,
                                   torch.float16, torch.int64])
def test_dump_rejects_unexpected_dtype(tmp_path, dtype):
    with pytest.raises(TypeError, match="unsupported dtype"):
        bench.dump_outputs(str(tmp_path / "o"),
                           {"x": torch.zeros(4, dtype=dtype)})


def _run_bench(monkeypatch, capsys, *argv):
    """bench.main() in-process (world size 1 needs no process group);
    returns the parsed JSON result line."""
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", *argv])
    capsys.readouterr()
    bench.main()
    lines = [ln for ln in capsys.readouterr().out.splitlines()
             if ln.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


@pytest.mark.gpu
def test_bench_dump_outputs_wiring(tmp_path, monkeypatch, capsys):
    """--dump-outputs through main(): the headline app's last-step ranks
    land in DIR/ranks.npy, sampled (4096 vertices over a 1024-value
    budget), identically positioned and equal-valued across two runs with
    the same arguments, and equal to the CPU reference after the same
    number of iterations. --steps sets the timed step count."""
    from lux_amd import cpu_ref
    from lux_amd.graph import Graph
    monkeypatch.setattr(bench, "DUMP_VALUE_BYTES", 4 * 1024)
    scale, ne, steps, warmup = 12, 40000, 3, 2
    outs = []
    for tag in ("a", "b"):
        d = str(tmp_path / tag)
        res = _run_bench(monkeypatch, capsys, "--steps", str(steps),
                         "--warmup", str(warmup), "--scale", str(scale),
                         "--edges", str(ne), "--seed", "7",
                         "--dump-outputs", d)
        assert res["steps"] == steps and res["warmup"] == warmup
        assert res["ms_per_step"] > 0 and res["metric"] == "GTEPS"
        assert "cc_labelprop" not in res["config"]
        assert sorted(os.listdir(d)) == ["ranks.npy", "ranks_index.npy"]
        outs.append((np.load(os.path.join(d, "ranks.npy")),
                     np.load(os.path.join(d, "ranks_index.npy"))))
    (ra, ia), (rb, ib) = outs
    assert ra.dtype == np.float32 and ra.shape == ia.shape == (1024,)
    np.testing.assert_array_equal(ia, ib)
    # fp32 atomic sum order differs run to run: same bound as smoke()
    np.testing.assert_allclose(ra, rb, rtol=1e-4, atol=1e-8)
    want = cpu_ref.pagerank(Graph.rmat(scale, ne, seed=7), steps + warmup)
    np.testing.assert_allclose(ra, want[ia.astype(np.int64)], rtol=1e-4,
                               atol=1e-8)


@pytest.mark.gpu
def test_bench_full_gates_cc_labelprop(tmp_path, monkeypatch, capsys):
    """--app cc: the label-propagation measurement is reported only with
    --full; both runs dump the same union-find labelling."""
    base = ("--app", "cc", "--steps", "1", "--warmup", "1", "--edges",
            "200000")
    d1, d2 = str(tmp_path / "plain"), str(tmp_path / "full")
    plain = _run_bench(monkeypatch, capsys, *base, "--dump-outputs", d1)
    full = _run_bench(monkeypatch, capsys, *base, "--full",
                      "--dump-outputs", d2)
    assert "cc_labelprop" not in plain["config"]
    lp = full["config"]["cc_labelprop"]
    assert lp["ms_per_step"] > 0 and lp["gteps"] > 0
    l1 = np.load(os.path.join(d1, "labels.npy"))
    assert l1.dtype == np.float64
    np.testing.assert_array_equal(l1, np.load(os.path.join(d2, "labels.npy")))
    np.testing.assert_array_equal(
        np.load(os.path.join(d1, "labels_index.npy")),
        np.load(os.path.join(d2, "labels_index.npy")))
