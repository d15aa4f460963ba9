"""TCEngine.clustering() on the GPU: per_vertex / C(deg, 2) from the
per-vertex triangle counts of src/gpu/tc.hip, against the dense-matrix
count and the simple degrees of tc_ref.py. The quotient of two exactly
represented integers is correctly rounded on both sides: equality."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import tc_ref  # noqa: E402
from lux_amd import _native_gpu as ng  # noqa: E402
from lux_amd import tc_engine as tce  # noqa: E402
from lux_amd.engine import DeviceCSC, GraphPart  # noqa: E402
from lux_amd.graph import Graph  # noqa: E402
from lux_amd.tc_engine import TCEngine  # noqa: E402


@pytest.fixture(autouse=True)
def native_lib_is_loaded():
    """The HIP extension must be the in-tree .so (no silent fallback)."""
    import lux_amd
    path = ng.lib()._name
    assert path.endswith("liblux_gpu.so")
    assert os.path.dirname(os.path.abspath(path)) == \
        os.path.dirname(os.path.abspath(lux_amd.__file__))


@pytest.fixture(autouse=True)
def default_knobs(monkeypatch):
    monkeypatch.delenv("LUX_TC_STAGE", raising=False)
    monkeypatch.delenv("LUX_TC_PLAIN", raising=False)


def want_clustering(g):
    _, pv, _ = tc_ref.dense_count(g)
    deg = tc_ref.simple_degrees(g)
    pairs = deg * (deg - 1) // 2
    return np.where(pairs > 0, pv / np.maximum(pairs, 1), 0.0)


@pytest.mark.parametrize("order", tce.ORDERS)
def test_clustering_rmat(order):
    g = Graph.rmat(10, 20000, seed=3, sym=True)
    want = want_clustering(g)
    eng = TCEngine(GraphPart(DeviceCSC.from_host(g, "cuda"), 1, 0),
                   order=order)
    got = eng.clustering()  # counts per vertex on first use
    assert got.dtype == torch.float64 and got.shape == (g.nv,)
    assert got.device.type == "cuda"
    assert np.array_equal(got.cpu().numpy(), want)
    assert 0.0 < want.max() <= 1.0 and (want == 0.0).any()


@pytest.mark.parametrize("name,value", [("k4", 1.0), ("star", 0.0),
                                        ("path", 0.0)])
def test_clustering_closed_forms(name, value):
    case = next(c for c in tc_ref.hand_cases() if c.name == name)
    eng = TCEngine(GraphPart(DeviceCSC.from_host(case.g, "cuda"), 1, 0))
    got = eng.clustering().cpu().numpy()
    assert np.array_equal(got, np.full(case.g.nv, value))
    assert np.array_equal(got, want_clustering(case.g))
